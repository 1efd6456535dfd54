"""Per-kernel fingerprint of the gfx950 code object inside each object file, sorted by symbol: SHA-256 of the kernel's
disassembly (llvm-objdump -d without addresses and encodings) and of its metadata note (registers, LDS, scratch, kernarg
size).  Where codeobj_hash.py differs between two builds, equal output here says that only the ORDER of the kernels moved.
    python profiles/tools/codeobj_kernels.py pram_amd/csrc/conv.o > after.txt      (then diff against the other build's)
"""
import hashlib, os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
run = lambda *a: subprocess.run(a, capture_output=True, text=True, check=True).stdout
sha = lambda lines: hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
with tempfile.TemporaryDirectory() as tmp:
    for f in sys.argv[1:]:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
        run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", f)
        run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
            f"--output={co}")
        text, cur = {}, None
        for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).split("\n"):
            m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
            if m:
                cur = text.setdefault(m.group(1), [])
            elif cur is not None:
                cur.append(re.sub(r"\s*//.*$", "", line).strip())      # the trailing comment holds the address
        meta = {}
        for blk in run(f"{LLVM}/llvm-readelf", "--notes", co).split("- .agpr_count:")[1:]:
            meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = [l.strip() for l in blk.split("\n")]
        for name in sorted(text):
            print(f"{os.path.basename(f)}  text {sha(text[name])}  meta {sha(meta[name]) if name in meta else '-':16s}  {name}")
