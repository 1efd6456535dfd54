"""CPU: the C ABI contract, once and by type.  Every function declared in include/pram_hip.h has the ctypes signature its
declaration maps to in pram_amd._lib._SIGS and is exported by the library, and every integer `#define PRAM_<NAME>` that
pram_amd.ops restates as <NAME> holds the header's value."""
import ctypes as C
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parents[1] / "include" / "pram_hip.h"
SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "float": C.c_float, "double": C.c_double,
           "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t}
# The (header, ops) constant pairs the test compares today.  The per-family tests compared 40 of them one by one before this test
# took them over: 14 PRAM_BA_*, 3 PRAM_BAC_*, 2 PRAM_COMPRESS_*, 3 PRAM_TRI_* and 3 PRAM_TRI_ROW_*, 2 PRAM_MAPBUILD_*, 4
# PRAM_KMEANS_*, 3 of knn.hip (PRAM_KNN_* / PRAM_SOR_BLOCK), 4 PRAM_IMGRET_*, PRAM_TWOVIEW_MAX_SOL and PRAM_MAP_MAX_LINKS.  A renamed
# constant drops out of the name match below; this floor is what notices, so it rises with every constant added.
MIN_CONSTANT_PAIRS = 49


def _code(header: str) -> str:
    """The header without comments and preprocessor lines."""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))


def _ctype(decl: str, is_return: bool = False):
    """The ctypes class of one parameter declaration (type and name) or of a return type."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        if is_return:
            assert words == ["char", "*"], decl      # the only pointer an entry returns is a string
            return C.c_char_p
        return C.c_void_p
    if not is_return:
        assert len(words) >= 2, f"parameter without a name: {decl!r}"
        words = words[:-1]
    return SCALARS[" ".join(words)]


def declarations(header: str) -> dict:
    """name -> (restype, [argtypes]) of every function declared in the header."""
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(pram_\w+)\s*\(([^()]*)\)\s*;", _code(header)):
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, f"{name} declared twice"
        out[name] = (_ctype(ret, True), [] if params in ("", "void") else [_ctype(p) for p in params.split(",")])
    return out


def test_parser_reads_every_form():
    decl = declarations("""
        /* int pram_commented(int a); */
        #define PRAM_X 3
        const char* pram_name(void);
        size_t pram_bytes(int n, unsigned flags, unsigned int* word,   // trailing
                          const double *x, long long ld, unsigned long long seed);
        float pram_scale(float s); int pram_two(double tol, void* stream);""")
    assert decl == {"pram_name": (C.c_char_p, []),
                    "pram_bytes": (C.c_size_t, [C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_longlong, C.c_ulonglong]),
                    "pram_scale": (C.c_float, [C.c_float]), "pram_two": (C.c_int, [C.c_double, C.c_void_p])}


def test_every_declaration_is_bound_with_its_types(hip_lib):
    from pram_amd import _lib
    decl = declarations(HEADER.read_text())
    assert len(decl) >= 24 and set(decl) == set(_lib.exported_symbols()), set(decl) ^ set(_lib.exported_symbols())
    # every mention of an entry followed by "(" in the header is one of the parsed declarations: the parser skipped none
    assert set(re.findall(r"\b(pram_[a-z0-9_]+)\s*\(", _code(HEADER.read_text()))) == set(decl)
    wrong = {n: (sig, _lib._SIGS[n]) for n, sig in decl.items() if (sig[0], list(sig[1])) != (_lib._SIGS[n][0], list(_lib._SIGS[n][1]))}
    assert not wrong, wrong
    missing = [n for n in decl if not hasattr(hip_lib, n)]
    assert not missing, missing


def test_constants_restated_in_ops_hold_the_headers_values():
    from pram_amd import ops
    # an integer in ops: PRAM_BA_ARRAYS and PRAM_BAC_ARRAYS count the tuples ops.BA_ARRAYS / ops.BAC_ARRAYS, which the bundle tests compare
    pairs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^[ \t]*#define PRAM_(\w+)[ \t]+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))[uU]?\)?[ \t]*(?:/\*.*|//.*)?$",
                                                                HEADER.read_text(), flags=re.M) if type(getattr(ops, m.group(1), None)) is int}
    wrong = {n: (v, getattr(ops, n)) for n, v in pairs.items() if getattr(ops, n) != v}
    assert not wrong, wrong
    assert len(pairs) >= MIN_CONSTANT_PAIRS, sorted(pairs)


ORDER_CHECK = """
import importlib, sys
first, second = sys.argv[1:3]
a, b = importlib.import_module(first), importlib.import_module(second)
ops, geo = (a, b) if first.endswith(".ops") else (b, a)
own = [k for k, v in vars(geo).items() if not k.startswith("__") and getattr(v, "__module__", geo.__name__) == geo.__name__ and type(v) is not type(sys)]
assert len(own) > 150 and all(getattr(ops, k) is getattr(geo, k) for k in own), [k for k in own if getattr(ops, k, None) is not getattr(geo, k)]
assert geo._st is ops._st and geo._chk is ops._chk and geo._filled is ops._filled and geo._workspace is ops._workspace
assert ops.imgret_topk.__module__ == geo.__name__ and ops.linear.__module__ == ops.__name__
"""


def test_ops_reexports_ops_geometry_in_either_import_order():
    """pram_amd.ops and pram_amd.ops_geometry import each other as their last statements: whichever comes first, every name the
    second defines is the same object under ops, and the primitives and the scratch cache are the first's, not copies."""
    import subprocess
    import sys
    root = HEADER.parents[1]
    for order in (("pram_amd.ops", "pram_amd.ops_geometry"), ("pram_amd.ops_geometry", "pram_amd.ops")):
        r = subprocess.run([sys.executable, "-c", ORDER_CHECK, *order], cwd=root, capture_output=True, text=True)
        assert r.returncode == 0, (order, r.stderr[-2000:])
