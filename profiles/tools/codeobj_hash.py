"""SHA-256 of the gfx950 code object inside each object file: equal hashes before and after a host-only change prove that no
kernel, argument-struct layout or instantiation moved — no GPU needed.  One line per file: "<sha256>  <name>".
    python profiles/tools/codeobj_hash.py [pram_amd/csrc/linear.o ...]      (default: every .o under pram_amd/csrc)
"""
import glob, hashlib, os, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
files = sys.argv[1:] or sorted(glob.glob(os.path.join(ROOT, "pram_amd", "csrc", "*.o")))
run = lambda *a: subprocess.run(a, capture_output=True, text=True, check=True)
with tempfile.TemporaryDirectory() as tmp:
    for f in files:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
        run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", f)
        run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
            f"--output={co}")
        with open(co, "rb") as fh:
            print(hashlib.sha256(fh.read()).hexdigest() + "  " + os.path.basename(f))
