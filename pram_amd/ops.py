"""Torch-facing wrappers over the C ABI (include/pram_hip.h).  PyTorch here is plumbing only:
device memory (torch.empty), the current HIP stream, and nothing else — every op below is a
hand-written gfx950 kernel in pram_amd/csrc.  All tensors must be fp32 CUDA tensors."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

_INT64 = torch.int64


def _st() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise _lib.PramHipError(f"{name}: expected a CUDA tensor (pram_amd has no CPU path)")
    if t.dtype != dtype:
        raise _lib.PramHipError(f"{name}: expected {dtype}, got {t.dtype}")


def _rows2d(t: torch.Tensor, name: str) -> Tuple[int, int]:
    """(rows, ld) of a tensor viewed as a row-major matrix over its last dim."""
    _chk(t, name)
    if t.stride(-1) != 1:
        raise _lib.PramHipError(f"{name}: last dim must be contiguous")
    return t.numel() // t.shape[-1], t.shape[-1]


def _rotary_args(rotary):
    """(flags, cos, sin, rot_cols) of a linear entry from the wrappers' optional (cos, sin, rot_cols) triple."""
    if rotary is None:
        return 0, None, None, 0
    rc, rs, rcols = rotary
    return 1, rc, rs, rcols


def _concat_rows(x: torch.Tensor, x2: Optional[torch.Tensor]):
    """x (and the optional second input segment x2) as contiguous row matrices -> (x, x2, m, k0, k1)."""
    x = x.contiguous()
    m, k0 = _rows2d(x, "x")
    k1 = 0
    if x2 is not None:
        x2 = x2.contiguous()
        m2, k1 = _rows2d(x2, "x2")
        assert m2 == m
    return x, x2, m, k0, k1


def _filled(shape, device, dtype=torch.float32, word: int = 0) -> torch.Tensor:
    """torch.zeros / torch.full for 32-bit dtypes without a framework kernel: torch.empty + hipMemsetD32Async on the current stream
    (``word`` = the 32-bit pattern; -2 as int32 is 0xFFFFFFFE)."""
    t = torch.empty(shape, device=device, dtype=dtype)
    assert t.element_size() == 4
    if t.numel():
        _lib.check(_lib.load().pram_fill_u32(t.data_ptr(), word & 0xFFFFFFFF, t.numel(), _st()), "pram_fill_u32")
    return t


def last_kernel() -> str:
    """The kernel instantiation the calling thread's last GEMM / convolution / attention launch took (pram_last_kernel), e.g.
    'linear_x3w<4,2,4>': the entries choose it from the launch grid.  '' before the first such launch."""
    return (_lib.load().pram_last_kernel() or b"").decode()


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, x2: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, alpha: float = 1.0, out: Optional[torch.Tensor] = None,
           rotary: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, half_copy: str = "no", split_out: str = "no",
           precision: Optional[str] = None, lens: Optional[torch.Tensor] = None, t_pad: int = 0, out_planes=None):
    """out = alpha * ([x | x2] @ w.T + bias) + residual.  x [..., k0] (contiguous rows), w [n, k0+k1].
    precision: None = ops.gemm_precision; "f32" exact-fp32 MFMA, "x3" split-fp16 (three fp16 MFMAs per product, fp32-class
    accuracy), "f16" single fp16 product (BASELINE C5).  Shapes a fast path cannot take (K not a multiple of 32 / 64)
    run on the exact-fp32 kernel.
    half_copy (f16 path only): "also" -> returns (out fp32, out fp16), "only" -> returns (None, out fp16): the fp16 operand
    of attention_h16.
    split_out (x3 path only): "also" -> (out fp32, (hi, lo)), "only" -> (None, (hi, lo)): the result * 16 as two fp16 planes,
    the operand format of attention_x3.
    lens / t_pad (every path; with half_copy the fp16 copy is dense): ragged token matrix — rows are sequences of t_pad rows with lens[s] valid ones; output tiles
    without a valid row are skipped and left untouched (and only valid rows are stored).
    out_planes (with split_out): a (hi, lo) pair of existing fp16 buffers to write into instead of fresh ones."""
    L = _lib.load()
    x, x2, m, k0, k1 = _concat_rows(x, x2)
    if lens is not None:
        assert t_pad > 0 and m % t_pad == 0 and lens.dtype == torch.int32 and lens.numel() == m // t_pad
    _chk(w, "w")
    w = w.contiguous()
    n = w.shape[0]
    assert w.shape[1] == k0 + k1, (w.shape, k0, k1)
    prec = _check_precision(_tl("forced") or precision or gemm_prec())
    want32 = not (half_copy == "only" or split_out == "only")
    if out is None and want32:
        out = torch.empty(*x.shape[:-1], n, device=x.device, dtype=torch.float32)
    if residual is not None:
        residual = residual.contiguous()
    flags, rc, rs, rcols = _rotary_args(rotary)
    K = k0 + k1
    use16 = prec == "f16" and K % 64 == 0 and (k1 == 0 or k0 % 64 == 0)
    x3_shape = K % 32 == 0 and (k1 == 0 or k0 % 32 == 0)
    usex3 = prec == "x3" and x3_shape
    if half_copy != "no":
        if not use16:
            raise _lib.PramHipError("linear(half_copy=...) needs the fp16 GEMM path (precision 'f16', K % 64 == 0)")
        out16 = torch.empty(*x.shape[:-1], n, device=x.device, dtype=torch.float16)
        o32 = out if half_copy == "also" else None
        if m:
            _lib.check(L.pram_linear_f16_h16(_p(x), k0, k0, _p(x2), k1, k1, _p(_w16(w)), _p(bias), _p(residual), n, _p(o32), n,
                                             _p(out16), n, m, n, float(alpha), flags, _p(rc), _p(rs), int(rcols), _st()),
                       "pram_linear_f16_h16")
        return o32, out16
    if split_out != "no":
        if not usex3:
            raise _lib.PramHipError("linear(split_out=...) needs the split-fp16 GEMM path (precision 'x3', K % 32 == 0)")
        if out_planes is not None:      # persistent plane buffers (AdaGML commits the rows of the pairs stopping at a layer)
            planes = out_planes
            assert planes[0].dtype == torch.float16 and planes[0].is_contiguous() and planes[1].is_contiguous() and planes[0].shape[-1] == n
        else:
            planes = torch.empty(2, *x.shape[:-1], n, device=x.device, dtype=torch.float16)
        o32 = out if split_out == "also" else None
        if m:
            wh, wl, ws = split_weight(w)
            _lib.check(L.pram_linear_x3_ragged_f32(_p(x), k0, k0, _p(x2), k1, k1, _p(wh), _p(wl), ws, _p(bias), _p(residual), n,
                                                   _p(o32), n, _p(planes[0]), _p(planes[1]), n, m, n, float(alpha), flags, _p(rc), _p(rs),
                                                   int(rcols), _p(lens), int(t_pad), _st()), "pram_linear_x3_ragged_f32")
        return o32, (planes[0], planes[1])
    if m == 0:          # empty token set: nothing to launch (an empty tensor has a null data pointer)
        return out
    if usex3:
        wh, wl, ws = split_weight(w)
        _lib.check(L.pram_linear_x3_ragged_f32(_p(x), k0, k0, _p(x2), k1, k1, _p(wh), _p(wl), ws, _p(bias), _p(residual), n, _p(out), n,
                                               None, None, 0, m, n, float(alpha), flags, _p(rc), _p(rs), int(rcols), _p(lens), int(t_pad),
                                               _st()), "pram_linear_x3_ragged_f32")
        return out
    if use16:      # ragged calls included: tiles without a valid row are skipped, only valid rows are stored (as on the other paths)
        _lib.check(L.pram_linear_f16_ragged_f32(_p(x), k0, k0, _p(x2), k1, k1, _p(_w16(w)), _p(bias), _p(residual),
                                                n, _p(out), n, m, n, float(alpha), flags, _p(rc), _p(rs), int(rcols), _p(lens), int(t_pad), _st()),
                   "pram_linear_f16_ragged_f32")
        return out
    _lib.check(L.pram_linear_ragged_f32(_p(x), k0, k0, _p(x2), k1, k1, _p(w), _p(bias), _p(residual),
                                        n, _p(out), n, m, n, float(alpha), flags, _p(rc), _p(rs), int(rcols), _p(lens), int(t_pad), _st()),
               "pram_linear_ragged_f32")
    return out


def mlp_tail(x: torch.Tensor, w0c: torch.Tensor, b0c: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w3: torch.Tensor,
             b3: Optional[torch.Tensor], *, x2: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
             eps: float = 1e-5, lens: Optional[torch.Tensor] = None, t_pad: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """residual + Linear(w3, b3)(GELU(LayerNorm(Linear(w0, b0)([x | x2])))) on the split-fp16 path as TWO kernels: the first GEMM
    (w0c / b0c = the weights centred over their outputs, center_linear()) writes h - mean(h) and the rows' sums of squares, the
    second normalises and GELUs its operand while it stages it (pram_linear_x3_ssq_f32 / pram_linear_x3_lngelu_f32).  Shapes the
    fast path cannot take (K % 32 != 0, hidden > 1024) raise."""
    L = _lib.load()
    x, x2, m, k0, k1 = _concat_rows(x, x2)
    hid = w0c.shape[0]
    n = w3.shape[0]
    if (k0 + k1) % 32 or (k1 and k0 % 32) or hid % 32 or hid > 1024 or w0c.shape[1] != k0 + k1 or w3.shape[1] != hid:
        raise _lib.PramHipError(f"mlp_tail: unsupported shapes K={k0}+{k1}, hidden={hid}")
    if lens is not None:
        assert t_pad > 0 and m % t_pad == 0 and lens.dtype == torch.int32 and lens.numel() == m // t_pad
    if out is None:
        out = torch.empty(*x.shape[:-1], n, device=x.device, dtype=torch.float32)
    if m == 0:
        return out
    parts = int(L.pram_linear_x3_ssq_parts(m, hid, k0 + k1))
    h = torch.empty(m, hid, device=x.device, dtype=torch.float32)
    ssq = torch.empty(parts, m, device=x.device, dtype=torch.float32)
    wh, wl, ws = split_weight(w0c.contiguous())
    _lib.check(L.pram_linear_x3_ssq_f32(_p(x), k0, k0, _p(x2), k1, k1, _p(wh), _p(wl), ws, _p(b0c), _p(h), hid, _p(ssq), m, hid,
                                        _p(lens), int(t_pad), _st()), "pram_linear_x3_ssq_f32")
    if residual is not None:
        residual = residual.contiguous()
    wh, wl, ws = split_weight(w3.contiguous())
    _lib.check(L.pram_linear_x3_lngelu_f32(_p(h), hid, hid, _p(wh), _p(wl), ws, _p(b3), _p(residual), n, _p(out), n, m, n, _p(ssq), parts,
                                           _p(gamma), _p(beta), float(eps), _p(lens), int(t_pad), _st()), "pram_linear_x3_lngelu_f32")
    return out


def center_linear(w: torch.Tensor, b: torch.Tensor):
    """(w - mean over the outputs, b - mean) in fp64 -> fp32: a Linear whose output is h - mean(h).  LayerNorm(h) only needs the
    centred values (it is invariant to the shift), so a Linear that feeds a LayerNorm can be centred once at pack time."""
    wd, bd = w.detach().double().cpu(), b.detach().double().cpu()
    return (wd - wd.mean(0, keepdim=True)).float().contiguous(), (bd - bd.mean()).float().contiguous()


def linear_qkv_planes(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], heads: int, t_seq: int,
                      rotary: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, lens: Optional[torch.Tensor] = None):
    """The q | k | v (or qk | v) projection of an attention block on the split-fp16 path, values written transposed:
    -> ((hi, lo) row-major planes [m, n - heads * 64] of the q / k columns, (vt_hi, vt_lo) = value_planes_t of the value columns).
    Rows are sequences of t_seq tokens (t_seq % 64 == 0); lens as in linear()."""
    L = _lib.load()
    x = x.contiguous()
    m, k0 = _rows2d(x, "x")
    n = w.shape[0]
    col0 = n - heads * 64
    assert t_seq % 64 == 0 and m % t_seq == 0 and k0 % 32 == 0 and col0 > 0 and col0 % 64 == 0
    planes = torch.empty(2, m, col0, device=x.device, dtype=torch.float16)
    vt = torch.empty(2, m // t_seq, heads, 64, t_seq, device=x.device, dtype=torch.float16)
    flags, rc, rs, rcols = _rotary_args(rotary)
    if m:
        wh, wl, ws = split_weight(w.contiguous())
        _lib.check(L.pram_linear_x3_qkv_f32(_p(x), k0, k0, _p(wh), _p(wl), ws, _p(bias), _p(planes[0]), _p(planes[1]), col0, _p(vt[0]), _p(vt[1]),
                                            col0, heads, t_seq, m, n, flags, _p(rc), _p(rs), int(rcols), _p(lens), _st()), "pram_linear_x3_qkv_f32")
    return (planes[0], planes[1]), (vt[0], vt[1])


def linear_planes(x, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, x2=None, residual: Optional[torch.Tensor] = None,
                  alpha: float = 1.0, rotary: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, out: str = "f32"):
    """linear() on the split-fp16 path with the activations ALREADY split: x (and x2) are (hi, lo) pairs of fp16 2-D views
    (value * s = hi + lo, s = the activation scale in force: 16 unless a model / act_scale_scope lowered it) written by a producing kernel's epilogue.  out: "f32" -> fp32 tensor; "planes" -> (hi, lo) planes of
    the result * s; "both" -> (fp32, (hi, lo))."""
    L = _lib.load()
    xh, xl = x
    assert xh.dtype == torch.float16 and xh.dim() == 2 and xh.stride(1) == 1 and xh.stride(0) == xl.stride(0)
    m, k0 = xh.shape
    k1 = 0
    if x2 is not None:
        assert x2[0].shape[0] == m and x2[0].stride(1) == 1 and x2[0].stride(0) == x2[1].stride(0)
        k1 = x2[0].shape[1]
    w = w.contiguous()
    n = w.shape[0]
    assert w.shape[1] == k0 + k1 and k0 % 32 == 0 and k1 % 32 == 0
    o32 = torch.empty(m, n, device=xh.device, dtype=torch.float32) if out in ("f32", "both") else None
    planes = torch.empty(2, m, n, device=xh.device, dtype=torch.float16) if out in ("planes", "both") else None
    flags, rc, rs, rcols = _rotary_args(rotary)
    if residual is not None:
        residual = residual.contiguous()
    if m:
        wh, wl, ws = split_weight(w)
        _lib.check(L.pram_linear_x3p_f32(_p(xh), _p(xl), xh.stride(0), k0, _p(x2[0]) if k1 else None, _p(x2[1]) if k1 else None,
                                         x2[0].stride(0) if k1 else 0, k1, _p(wh), _p(wl), ws, _p(bias), _p(residual), n, _p(o32), n,
                                         _p(planes[0]) if planes is not None else None, _p(planes[1]) if planes is not None else None,
                                         n, m, n, float(alpha), flags, _p(rc), _p(rs), int(rcols), _st()), "pram_linear_x3p_f32")
    pl = None if planes is None else (planes[0], planes[1])
    return o32 if out == "f32" else (pl if out == "planes" else (o32, pl))


def bgemm_nt(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0, ldc: Optional[int] = None) -> torch.Tensor:
    """c[z] = alpha * a[z] @ b[z].T ; a [B,M,K], b [B,N,K] -> c [B,M,ldc] (view [:, :, :N] is the result)."""
    L = _lib.load()
    a, b = a.contiguous(), b.contiguous()
    _chk(a, "a"), _chk(b, "b")
    B, M, K = a.shape
    N = b.shape[1]
    ldc = ldc or N
    c = torch.empty(B, M, ldc, device=a.device, dtype=torch.float32)
    _lib.check(L.pram_bgemm_nt_f32(_p(a), K, M * K, _p(b), K, N * K, _p(c), ldc, M * ldc, B, M, N, K, float(alpha), _st()),
               "pram_bgemm_nt_f32")
    return c


def bgemm_nt_planes(a, b, batch: int, m: int, n: int, alpha: float = 1.0, ldc: Optional[int] = None) -> torch.Tensor:
    """bgemm_nt on the split-fp16 path: a / b are (hi, lo) pairs of fp16 2-D views [batch * m, K] / [batch * n, K] (value * 16 =
    hi + lo, e.g. row ranges of linear(split_out=...)'s planes) -> c [batch, m, ldc] fp32."""
    L = _lib.load()
    for pair in (a, b):
        for t in pair:
            assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1
        assert pair[0].stride(0) == pair[1].stride(0)
    K = a[0].shape[1]
    assert b[0].shape[1] == K and b[0].stride(0) == K and a[0].shape[0] == batch * m and b[0].shape[0] == batch * n
    ldc = ldc or n
    c = torch.empty(batch, m, ldc, device=a[0].device, dtype=torch.float32)
    lda = a[0].stride(0)
    _lib.check(L.pram_bgemm_nt_x3p_f32(_p(a[0]), _p(a[1]), lda, m * lda, _p(b[0]), _p(b[1]), K, n * K, _p(c), ldc, m * ldc, batch, m, n, K,
                                       float(alpha), _st()), "pram_bgemm_nt_x3p_f32")
    return c


def layernorm_gelu_(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
                    lens: Optional[torch.Tensor] = None, t_pad: int = 0) -> torch.Tensor:
    L = _lib.load()
    rows, cols = _rows2d(x, "x")
    assert x.is_contiguous()
    _lib.check(L.pram_layernorm_gelu_ragged_f32(_p(x), cols, _p(x), cols, _p(gamma), _p(beta), rows, cols, float(eps), _p(lens), int(t_pad),
                                                _st()), "pram_layernorm_gelu_ragged_f32")
    return x


def fourier_encoding(kpts: torch.Tensor, wr: torch.Tensor, cx: float, cy: float, scale: float, out=None):
    """kpts [..., 2] -> (cos, sin) [..., 32]; out: a (cos, sin) pair of contiguous [rows, 32] views to write into."""
    L = _lib.load()
    kpts = kpts.contiguous().float()
    _chk(kpts, "kpts")
    rows = kpts.numel() // 2
    if out is not None:
        cos, sin = out
        assert cos.is_contiguous() and sin.is_contiguous() and cos.numel() == rows * 32 and sin.numel() == rows * 32
    else:
        cos = torch.empty(*kpts.shape[:-1], 32, device=kpts.device, dtype=torch.float32)
        sin = torch.empty_like(cos)
    _lib.check(L.pram_fourier_encoding_f32(_p(kpts), _p(wr), float(cx), float(cy), float(scale), _p(cos), _p(sin), rows, _st()),
               "pram_fourier_encoding_f32")
    return cos, sin


# bench.py's roofline probe: when set to a list, every attention launch is bracketed by HIP events on the
# launch stream and (algorithmic flops, start, stop) is appended.  None (default) = no events.
attention_probe = None

# MFMA path of the three matrix families (token GEMMs + convolutions / attention):
#   "f32" exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: the f32 vector rate);
#   "x3"  split-fp16: every fp32 operand = hi + lo in fp16, three v_mfma_f32_32x32x16_f16 per product, fp32 accumulate —
#         fp32-class accuracy (passes the same 1e-3 / indices-exact gates) at 5.3x less matrix time;
#   "f16" single fp16 product (BASELINE config C5's "fp16 MFMA path", own documented tolerance).
# Process defaults come from PRAM_PRECISION (both) or PRAM_GEMM_PRECISION / PRAM_ATTENTION_PRECISION; every op also takes
# an explicit ``precision=`` and every model a ``.precision`` attribute that overrides them.
import os as _os
import weakref as _weakref
PRECISIONS = ("f32", "x3", "f16")
default_precision = _os.environ.get("PRAM_PRECISION", "x3")
attention_precision = _os.environ.get("PRAM_ATTENTION_PRECISION", default_precision)
gemm_precision = _os.environ.get("PRAM_GEMM_PRECISION", default_precision)


def _check_precision(p: str) -> str:
    if p not in PRECISIONS:
        raise _lib.PramHipError(f"unknown precision {p!r} (expected one of {PRECISIONS})")
    return p


def set_precision(p: str) -> None:
    """Process-wide default for both the GEMM / convolution family and the attention family (thread-local scopes override it)."""
    global attention_precision, gemm_precision
    attention_precision = gemm_precision = _check_precision(p)


def current_precision() -> str:
    g, a = gemm_prec(), attn_prec()
    return a if a == g else f"gemm {g} / attention {a}"


import threading as _threading

# Scopes (precision_scope / forced_precision / guard_scope) and the guard's nesting depth are PER HOST THREAD: a process that drives
# several GPUs from one thread each must not see another thread's model-level override or nesting depth.  The module attributes
# gemm_precision / attention_precision / x3_guard stay the process-wide DEFAULTS (what set_precision() and the environment set);
# gemm_prec() / attn_prec() / guard_policy() return what is in force for the calling thread.
_tls = _threading.local()


def _tl(name, default=None):
    return getattr(_tls, name, default)


def gemm_prec() -> str:
    """MFMA path of the token GEMMs / convolutions in force for the calling thread (scope override, else the process default)."""
    return _tl("forced") or _tl("gemm") or gemm_precision


def attn_prec() -> str:
    """MFMA path of the attention family in force for the calling thread."""
    return _tl("forced") or _tl("attn") or attention_precision


def guard_policy() -> str:
    return _tl("guard") or x3_guard


class forced_precision:
    """``with ops.forced_precision("f32"): ...`` — every op and every model this thread runs inside the block uses that MFMA
    path, whatever the models' own ``.precision`` says (the range guard's fallback run)."""

    def __init__(self, p: str):
        self.p = _check_precision(p)

    def __enter__(self):
        self.saved = _tl("forced")
        _tls.forced = self.p

    def __exit__(self, *exc):
        _tls.forced = self.saved
        return False


class precision_scope:
    """``with ops.precision_scope("x3"): ...`` — what a model with a ``.precision`` attribute wraps its forward in (None: no
    override).  Thread-local; an enclosing forced_precision wins."""

    def __init__(self, p: Optional[str]):
        self.p = None if p is None else _check_precision(p)

    def __enter__(self):
        self.saved = (_tl("gemm"), _tl("attn"))
        if self.p is not None:
            _tls.gemm = _tls.attn = self.p

    def __exit__(self, *exc):
        _tls.gemm, _tls.attn = self.saved
        return False


# ---- range guard of the split-fp16 path (include/pram_hip.h, "range guard").  Every x3 kernel that splits fp32 values reports
# a finite |value| >= 4094.97 (its hi part would be +-inf in fp16) in a device status word owned here, one per device.  Launches
# are asynchronous, so the word is read where the host synchronises anyway:
#   * the model entry points (forward / produce_matches / extract_*: nets/_blocks.with_model_precision) read it after their last
#     launch and, when it is set, re-run the call on the exact-fp32 kernels (x3_guard = "fallback", the default), raise
#     (x3_guard = "raise"), or leave it to the caller (x3_guard = "deferred": no synchronisation; ask x3_range_exceeded());
#   * pipeline.QueryPipeline does the same once per run; bench.py defers it to the end of the timed region and reports it.
# WHETHER there is anything to read is decided by what was launched, not by the precision settings: every binding that launches a
# splitting kernel marks its device (_mark_x3: all of them fetch their weight planes through split_weight), so a model that runs
# x3 under its own .precision inside an f32 process, or the x3 kernels the fp16 path uses on purpose (GML's matching descriptors),
# arm the guard all the same — and a pure f32 / f16 run never synchronises for it.
x3_guard = _os.environ.get("PRAM_X3_GUARD", "fallback")
X3_GUARDS = ("fallback", "raise", "deferred")
_status_words = {}
_x3_pending = set()       # device indices with split-fp16 launches since their status word was last read
_x3_counts = {}           # device index -> split-fp16 launches so far (x3_launch_count: what a hipGraph capture compares)


def _dev_index(device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _mark_x3(device) -> None:
    i = _dev_index(device)
    _x3_pending.add(i)
    _x3_counts[i] = _x3_counts.get(i, 0) + 1


def mark_x3(device) -> None:
    """For callers that re-issue captured work (hipGraph replays launch nothing through these bindings): arm the range guard's
    read for ``device`` without counting a launch — x3_launched() is True again until the status word is next read."""
    _x3_pending.add(_dev_index(device))


def x3_launch_count(device=None) -> int:
    """Split-fp16 launches issued (or captured) on ``device`` so far: a caller that replays captured work compares the count
    around the capture to know whether its replays can set the status word."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _x3_counts.get(_dev_index(device), 0)


def x3_launched(device=None) -> bool:
    """True if a split-fp16 kernel was launched on ``device`` since its status word was last read (no synchronisation)."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _dev_index(device) in _x3_pending


def _x3_status(device) -> torch.Tensor:
    """The status word of ``device`` (allocated and registered with the library on first use)."""
    key = _dev_index(device)
    w = _status_words.get(key)
    if w is None:
        with torch.cuda.device(key):
            w = torch.zeros(4, device=torch.device("cuda", key), dtype=torch.int32)
            _lib.check(_lib.load().pram_set_status_word(w.data_ptr()), "pram_set_status_word")
        _status_words[key] = w
    return w


def x3_range_exceeded(device=None, reset: bool = True) -> bool:
    """True if a split-fp16 kernel met a value beyond the format's range since the last reset (synchronises with the device:
    the kernels that could set the word have to be done)."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    w = _x3_status(device)
    torch.cuda.synchronize(device)
    _x3_pending.discard(_dev_index(device))      # everything launched so far has reported
    hit = bool(int(w[0].item()) & 1)
    if hit and reset:
        w.zero_()
    return hit


class guard_scope:
    """``with ops.guard_scope("deferred"): ...`` — the range-guard policy of the model calls this thread makes inside."""

    def __init__(self, mode: str):
        if mode not in X3_GUARDS:
            raise _lib.PramHipError(f"unknown x3 guard {mode!r} (expected one of {X3_GUARDS})")
        self.mode = mode

    def __enter__(self):
        self.saved = _tl("guard")
        _tls.guard = self.mode

    def __exit__(self, *exc):
        _tls.guard = self.saved
        return False


# ---- activation scale of the split-fp16 path (include/pram_hip.h, "activation scale").  The planes carry value * s, s = 16 by
# default (range |x| < 4094.97).  A model whose activations are larger — trained checkpoints — does not have to leave the split
# path: it lowers s (a power of two; s = 1 carries |x| < 65520, s = 1/16 a million) and keeps the same 22-bit significand.  The
# scale is a property of the MODEL (PackedCache.act_scale, applied around its forward by nets/_blocks.with_model_precision) and
# is found by the range guard itself: a tripped guard first lowers the scale of the models that ran (sticky: the cliff is met
# once) and re-runs on the split kernels; only a value no scale can carry goes to the exact-fp32 kernels.
ACT_SCALE_DEFAULT = 16.0
ACT_SCALE_MIN = 2.0 ** -8      # the guard lowers EVERY model that ran: all of them keep their bars down to here (tests/test_gpu_act_scale.py)
guard_events = {"rescaled": 0, "f32_fallback": 0}      # what the range guard did so far in this process (tests / bench read it)


def current_act_scale() -> float:
    return float(_lib.load().pram_x3_set_act_scale(0.0))


class act_scale_scope:
    """``with ops.act_scale_scope(s): ...`` — the split-fp16 launches of this thread inside the block carry their activation planes
    as value * s (None: no change).  Producers and consumers of planes must run under the same scale."""

    def __init__(self, s: Optional[float]):
        self.s = None if s is None else float(s)

    def __enter__(self):
        self.saved = None
        if self.s is not None:
            self.saved = float(_lib.load().pram_x3_set_act_scale(self.s))
            if self.saved < 0:
                raise _lib.PramHipError(f"activation scale {self.s!r}: expected a power of two in [2^-12, 16]")

    def __exit__(self, *exc):
        if self.saved is not None:
            _lib.load().pram_x3_set_act_scale(self.saved)
        return False


def _ran_models():
    """models (PackedCache) whose guarded forward ran inside the current outermost guarded call of this thread"""
    return _tl("ran", None)


def note_model_ran(model) -> None:
    ran = _tl("ran", None)
    if ran is not None and all(m is not model for m in ran):
        ran.append(model)


def guarded_call(fn, device):
    """Run ``fn()`` (a model entry point) under the range guard: only the OUTERMOST guarded call of a thread checks the status
    word, after its last launch, and only if a split-fp16 kernel was launched on the device since the word was last read; nothing
    is checked while a stream is capturing (a hipGraph cannot synchronise: GraphedPipeline checks after the replay).
    A tripped guard ("fallback", the default) first divides the activation scale of every model that ran inside the call by 16
    (down to ACT_SCALE_MIN; the models keep it) and re-runs on the split kernels; when no scale is left to give, or nothing that
    ran has one, the call re-runs on the exact-fp32 kernels."""
    depth = _tl("depth", 0)
    if depth == 0:
        _tls.ran = []
    _tls.depth = depth + 1
    try:
        out = fn()
    finally:
        _tls.depth = depth
    policy = guard_policy()
    if depth != 0:
        return out
    ran, _tls.ran = _tl("ran", None) or [], None
    if policy == "deferred" or not x3_launched(device):
        return out
    if policy not in X3_GUARDS:
        raise _lib.PramHipError(f"unknown x3 guard {policy!r} (expected one of {X3_GUARDS})")
    if torch.cuda.is_current_stream_capturing() or not x3_range_exceeded(device):
        return out
    if policy == "raise":
        raise _lib.PramHipError("split-fp16 path: an activation beyond the range of its planes (|x| >= 65520 / act_scale; "
                                "4094.97 at the default scale) — lower the models' act_scale, or re-run with precision 'f32' "
                                "(PRAM_X3_GUARD=fallback does both by itself)")
    while True:
        scalable = [m for m in ran if getattr(m, "act_scale", None) and m.act_scale / 16.0 >= ACT_SCALE_MIN]
        if not scalable:
            break
        for m in scalable:
            m.act_scale = m.act_scale / 16.0
        guard_events["rescaled"] += 1
        _tls.depth, _tls.ran = depth + 1, None
        try:
            out = fn()
        finally:
            _tls.depth = depth
        if not x3_range_exceeded(device):
            return out
    guard_events["f32_fallback"] += 1
    _tls.depth = depth + 1
    try:
        with forced_precision("f32"):
            return fn()
    finally:
        _tls.depth = depth


# Derived forms of a (static) weight tensor — its fp16 copy, its split planes — live exactly as long as the tensor object
# they were derived from and are rebuilt when it is modified in place (tensor._version), never keyed by a device address
# that the allocator may hand to another tensor.
_derived_cache = {}


def _derived(w: torch.Tensor, kind: str, fn):
    ent = _derived_cache.get(id(w))
    if ent is None or ent[0]() is not w or ent[1] != w._version:
        key = id(w)
        ent = (_weakref.ref(w, lambda _r, k=key: _derived_cache.pop(k, None)), w._version, {})
        _derived_cache[key] = ent
    v = ent[2].get(kind)
    if v is None:
        with torch.no_grad():
            v = ent[2][kind] = fn(w)
    return v


def _w16(w: torch.Tensor) -> torch.Tensor:
    """fp16 copy of a (static) weight tensor."""
    return _derived(w, "h16", lambda t: t.half().contiguous())


def split_weight_raw(t: torch.Tensor):
    """(hi, lo, scale) of a tensor, uncached: see split_weight."""
    import math
    amax = float(t.abs().max())
    scale = 2.0 ** math.floor(math.log2(16384.0 / amax)) if amax > 0 and math.isfinite(amax) else 1.0
    ts = t.float() * scale
    hi = ts.half()
    lo = (ts - hi.float()).half()
    return hi.contiguous(), lo.contiguous(), float(scale)


def split_weight(w: torch.Tensor):
    """-> (hi, lo, scale): w * scale = hi + lo as two fp16 tensors of w's shape; scale = the power of two that puts
    max|w| into [2^13, 2^14) (exact to apply and to undo), so hi + lo carries 22 bits of every weight above 2^-17 max|w|."""
    make = split_weight_raw
    _x3_status(w.device)      # every split-fp16 GEMM / convolution comes through here: the range guard's status word is registered,
    _mark_x3(w.device)        # and the device is marked as having something to report (guarded_call / x3_launched)
    return _derived(w, "x3", make)


attention_split = True      # False: never hand the kernel a split workspace (tests compare both modes bit for bit)


def _attention_ws(L, batch, heads, m_max, n_max, device):
    """workspace for the split (small-launch) mode, per stream: two streams may run attention concurrently"""
    nb = int(L.pram_attention_workspace_bytes(batch, heads, m_max, n_max)) if attention_split else 0
    if nb == 0:
        return None, 0
    return _workspace(nb, device, "attention"), nb


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, heads: int, m_max: int, n_max: int,
              scale: float, q_lens: Optional[torch.Tensor] = None, k_lens: Optional[torch.Tensor] = None,
              want_lse: bool = False, out: Optional[torch.Tensor] = None, precision: Optional[str] = None):
    """q/k/v: 2-D row-major views (possibly column slices of a wider buffer): q [batch*m_max, >=heads*64]."""
    L = _lib.load()
    for t, nm in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, nm)
        assert t.dim() == 2 and t.stride(1) == 1
    if out is None:
        out = torch.empty(batch * m_max, heads * 64, device=q.device, dtype=torch.float32)
    lse = torch.empty(batch, heads, m_max, device=q.device, dtype=torch.float32) if want_lse else None
    probe = attention_probe
    if probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    prec = _check_precision(_tl("forced") or precision or attn_prec())
    if prec == "x3":
        prec = "f32"      # fp32 operands in HBM: the split path starts at the projection (attention_x3 takes its planes)
    if prec == "f32":
        ws, nb = _attention_ws(L, batch, heads, m_max, n_max, q.device)
        rc = L.pram_attention_f32(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                  _p(lse), _p(q_lens), _p(k_lens), batch, heads, m_max, n_max, float(scale), _p(ws), nb, _st())
    else:
        rc = L.pram_attention_f16_f32(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                      _p(lse), _p(q_lens), _p(k_lens), batch, heads, m_max, n_max, float(scale), _st())
    _lib.check(rc, "pram_attention_f32" if prec == "f32" else "pram_attention_f16_f32")
    if probe is not None:
        e1.record()
        # algorithmic FLOPs of QK^T + PV: 4 * m_b * n_b * 64 per (batch element, head), from the ACTUAL ragged
        # lengths (device tensors, summed by the caller after synchronising)
        probe.append((q_lens, k_lens, m_max, n_max, heads, batch, e0, e1, "self", 16))
    return (out, lse) if want_lse else out


def attention_colmean(q: torch.Tensor, k: torch.Tensor, lse2: torch.Tensor, batch: int, heads: int, m_max: int,
                      n_max: int, scale: float, q_lens=None, k_lens=None) -> torch.Tensor:
    L = _lib.load()
    out = _filled((batch, n_max), q.device)
    _lib.check(L.pram_attention_colmean_f32(_p(q), q.stride(0), _p(k), k.stride(0), _p(lse2), _p(out), _p(q_lens),
                                            _p(k_lens), batch, heads, m_max, n_max, float(scale), _st()),
               "pram_attention_colmean_f32")
    return out


def attention_h16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, heads: int, m_max: int, n_max: int, scale: float,
                  q_lens: Optional[torch.Tensor] = None, k_lens: Optional[torch.Tensor] = None, want_lse: bool = False,
                  out: Optional[torch.Tensor] = None, kv_shift: int = 0):
    """attention(precision="f16") on fp16 q / k / v (2-D views, possibly column slices of one fp16 projection output):
    same bits out, half the operand traffic.  kv_shift: see attention_cross."""
    L = _lib.load()
    for t in (q, k, v):
        assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1
    if out is None:
        out = torch.empty(batch * m_max, heads * 64, device=q.device, dtype=torch.float32)
    lse = torch.empty(batch, heads, m_max, device=q.device, dtype=torch.float32) if want_lse else None
    probe = attention_probe
    if probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.check(L.pram_attention_h16_f32(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                        _p(lse), _p(q_lens), _p(k_lens), batch, heads, m_max, n_max, float(scale), int(kv_shift),
                                        _st()), "pram_attention_h16_f32")
    if probe is not None:
        e1.record()
        kl = k_lens if (k_lens is None or not kv_shift) else torch.roll(k_lens, -kv_shift)
        probe.append((q_lens, kl, m_max, n_max, heads, batch, e0, e1, "cross" if kv_shift else "self", 16))
    return (out, lse) if want_lse else out


def value_t16(v16: torch.Tensor, seqs: int, heads: int, t_max: int, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16 row-major values [seqs * t_max, >= heads * 64] -> the transposed, key-permuted fp16 values [seqs, heads, 64, tv] of
    attention_h16t (the single-plane form of value_planes_t)."""
    L = _lib.load()
    assert v16.is_cuda and v16.dtype == torch.float16 and v16.dim() == 2 and v16.stride(1) == 1
    tv = (t_max + 63) // 64 * 64
    out = torch.empty(seqs, heads, 64, tv, device=v16.device, dtype=torch.float16)
    _lib.check(L.pram_attention_x3_vt(_p(v16), None, v16.stride(0), _p(out), None, _p(lens), seqs, heads, t_max, _st()), "pram_attention_x3_vt")
    return out


def attention_h16t(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, batch: int, heads: int, m_max: int, n_max: int, scale: float,
                   q_lens: Optional[torch.Tensor] = None, k_lens: Optional[torch.Tensor] = None, want_lse: bool = False,
                   out: Optional[torch.Tensor] = None, kv_shift: int = 0):
    """The fp16 path's attention on the software-pipelined kernel: fp16 q / k (2-D views), vt = value_t16(...) of the key side.
    One fp16 MFMA per product, probabilities rounded to fp16 (tolerance of the fp16 path)."""
    L = _lib.load()
    for t in (q, k):
        assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1
    assert vt.is_contiguous() and vt.dtype == torch.float16
    if out is None:
        out = torch.empty(batch * m_max, heads * 64, device=q.device, dtype=torch.float32)
    # ragged queries: the kernel writes lse for the rows below q_lens[b] only; the rows beyond are 0, not what the allocator held
    lse = None if not want_lse else (torch.empty(batch, heads, m_max, device=q.device, dtype=torch.float32) if q_lens is None
                                     else _filled((batch, heads, m_max), q.device))
    probe = attention_probe
    if probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.check(L.pram_attention_h16t_f32(_p(q), q.stride(0), _p(k), k.stride(0), _p(vt), _p(out), out.stride(0), _p(lse), _p(q_lens),
                                         _p(k_lens), batch, heads, m_max, n_max, float(scale), int(kv_shift), _st()), "pram_attention_h16t_f32")
    if probe is not None:
        e1.record()
        kl = k_lens if (k_lens is None or not kv_shift) else torch.roll(k_lens, -kv_shift)
        probe.append((q_lens, kl, m_max, n_max, heads, batch, e0, e1, "cross" if kv_shift else "self", 16))
    return (out, lse) if want_lse else out


def value_planes_t(v, seqs: int, heads: int, t_max: int, lens: Optional[torch.Tensor] = None):
    """(hi, lo) row-major value planes [seqs * t_max, >= heads * 64] (column slices of linear(split_out=...)'s planes) ->
    the transposed, key-permuted planes [seqs, heads, 64, tv] attention_x3 stages with 16-byte copies; zeros beyond lens."""
    L = _lib.load()
    tv = (t_max + 63) // 64 * 64
    out = torch.empty(2, seqs, heads, 64, tv, device=v[0].device, dtype=torch.float16)
    assert v[0].stride(0) == v[1].stride(0) and v[0].stride(1) == 1 and v[0].dtype == torch.float16
    _lib.check(L.pram_attention_x3_vt(_p(v[0]), _p(v[1]), v[0].stride(0), _p(out[0]), _p(out[1]), _p(lens), seqs, heads, t_max, _st()),
               "pram_attention_x3_vt")
    return out[0], out[1]


def attention_x3(q, k, vt, batch: int, heads: int, m_max: int, n_max: int, scale: float,
                 q_lens: Optional[torch.Tensor] = None, k_lens: Optional[torch.Tensor] = None, want_lse: bool = False,
                 out: Optional[torch.Tensor] = None, kv_shift: int = 0):
    """Split-fp16 flash attention.  q / k: (hi, lo) pairs of fp16 2-D views (column slices of the planes written by
    linear(split_out=...)); vt: the (hi, lo) planes of value_planes_t for the key side.  fp32-class results, three fp16
    MFMAs per product.  kv_shift: see attention_cross."""
    L = _lib.load()
    for pair in (q, k):
        for t in pair:
            assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1
        assert pair[0].stride(0) == pair[1].stride(0)
    tv = (n_max + 63) // 64 * 64
    assert vt[0].is_contiguous() and vt[1].is_contiguous() and vt[0].dtype == torch.float16 and vt[0].numel() == batch * heads * 64 * tv
    if out is None:
        out = torch.empty(batch * m_max, heads * 64, device=q[0].device, dtype=torch.float32)
    lse = torch.empty(batch, heads, m_max, device=q[0].device, dtype=torch.float32) if want_lse else None
    probe = attention_probe
    if probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    # from 1024 keys on the keys are reduced in chunks; under-filled launches (one or two query frames) run the chunks as a grid
    # dimension through a workspace: same bits, shorter serial walk.  attention_split = False (tests): no workspace -> always fused.
    nb = int(L.pram_attention_x3_workspace_bytes(batch, heads, m_max, n_max)) if attention_split else 0
    ws = _workspace(nb, q[0].device, "attention_x3") if nb else None
    _x3_status(q[0].device)
    _lib.check(L.pram_attention_x3_f32(_p(q[0]), _p(q[1]), q[0].stride(0), _p(k[0]), _p(k[1]), k[0].stride(0), _p(vt[0]), _p(vt[1]),
                                       _p(out), out.stride(0), _p(lse), _p(q_lens), _p(k_lens), batch, heads,
                                       m_max, n_max, float(scale), int(kv_shift), _p(ws), nb, _st()), "pram_attention_x3_f32")
    if probe is not None:
        e1.record()
        kl = k_lens if (k_lens is None or not kv_shift) else torch.roll(k_lens, -kv_shift)
        probe.append((q_lens, kl, m_max, n_max, heads, batch, e0, e1, "cross" if kv_shift else "self",
                      int(L.pram_attention_x3_mfma_per_tile(n_max))))
    return (out, lse) if want_lse else out


def attention_colmean_x3(q, k, lse2: torch.Tensor, batch: int, heads: int, m_max: int, n_max: int, scale: float,
                         q_lens=None, k_lens=None, kv_shift: int = 0) -> torch.Tensor:
    """Column means of the soft-max matrix attention_x3 just produced (its q / k planes, its lse) -> [batch, n_max] fp32, row
    (b + kv_shift) % batch holding the means over sequence b's queries; keys beyond their length read 0."""
    L = _lib.load()
    for pair in (q, k):
        for t in pair:
            assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1
        assert pair[0].stride(0) == pair[1].stride(0)
    out = _filled((batch, n_max), lse2.device)
    _lib.check(L.pram_attention_x3_colmean_f32(_p(q[0]), _p(q[1]), q[0].stride(0), _p(k[0]), _p(k[1]), k[0].stride(0), _p(lse2), _p(out),
                                               _p(q_lens), _p(k_lens), batch, heads, m_max, n_max, float(scale), int(kv_shift), _st()),
               "pram_attention_x3_colmean_f32")
    return out


def attention_cross(qk: torch.Tensor, v: torch.Tensor, pairs: int, heads: int, t_max: int, scale: float,
                    lens: Optional[torch.Tensor] = None, want_lse: bool = False, out: Optional[torch.Tensor] = None,
                    precision: Optional[str] = None):
    """Both directions of the matcher's cross attention in one launch.  qk / v: [2*pairs*t_max, >= heads*64] row-major
    views; sequences 0..pairs-1 are set 0 and attend to set 1 (pairs..2*pairs-1) and vice versa.  lens int32 [2*pairs].
    Equal, bit for bit, to attention(qk0, qk1, v1) and attention(qk1, qk0, v0) written to the two halves of out."""
    L = _lib.load()
    for t, nm in ((qk, "qk"), (v, "v")):
        _chk(t, nm)
        assert t.dim() == 2 and t.stride(1) == 1
    S = 2 * pairs
    if out is None:
        out = torch.empty(S * t_max, heads * 64, device=qk.device, dtype=torch.float32)
    lse = torch.empty(S, heads, t_max, device=qk.device, dtype=torch.float32) if want_lse else None
    probe = attention_probe
    if probe is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    prec = _check_precision(_tl("forced") or precision or attn_prec())
    if prec == "x3":
        prec = "f32"
    if prec == "f32":
        ws, nb = _attention_ws(L, S, heads, t_max, t_max, qk.device)
        rc = L.pram_attention_cross_f32(_p(qk), qk.stride(0), _p(v), v.stride(0), _p(out), out.stride(0), _p(lse), _p(lens),
                                        pairs, heads, t_max, float(scale), _p(ws), nb, _st())
    else:
        rc = L.pram_attention_cross_f16_f32(_p(qk), qk.stride(0), _p(v), v.stride(0), _p(out), out.stride(0), _p(lse), _p(lens),
                                            pairs, heads, t_max, float(scale), _st())
    _lib.check(rc, "pram_attention_cross_f32" if prec == "f32" else "pram_attention_cross_f16_f32")
    if probe is not None:
        e1.record()
        probe.append((lens, None if lens is None else torch.roll(lens, -pairs), t_max, t_max, heads, S, e0, e1, "cross", 16))
    return (out, lse) if want_lse else out


def attention_cross_colmean(qk: torch.Tensor, lse2: torch.Tensor, pairs: int, heads: int, t_max: int, scale: float,
                            lens=None) -> torch.Tensor:
    """[2*pairs, t_max]: row kb = per token of sequence kb, mean attention received from the other set's queries."""
    L = _lib.load()
    out = _filled((2 * pairs, t_max), qk.device)
    _lib.check(L.pram_attention_cross_colmean_f32(_p(qk), qk.stride(0), _p(lse2), _p(out), _p(lens), pairs, heads, t_max,
                                                  float(scale), _st()), "pram_attention_cross_colmean_f32")
    return out


_ws_cache = {}
_ws_scopes = []          # innermost active workspace_scope store
_ws_captured = []        # scratch allocated while a stream was capturing outside any scope: owned by the process


class workspace_scope:
    """Route every scratch allocation of the enclosed launches into ``store`` (a dict owned by the caller) instead of
    the process-wide cache.  ``GraphedPipeline`` warms up and captures inside its own scope, so the pointers baked into
    its hipGraph belong to that graph alone: a later eager run that needs a larger workspace, or a second graph
    captured on torch's shared capture stream, can neither free nor share them.  A buffer that has to grow inside a
    scope is retired, not freed (an earlier capture may still point at it)."""

    def __init__(self, store: dict):
        self.store = store

    def __enter__(self):
        _ws_scopes.append(self.store)
        return self.store

    def __exit__(self, *exc):
        _ws_scopes.pop()
        return False


def _workspace(nbytes: int, device, tag: str = "") -> torch.Tensor:
    """Scratch memory owned by (device, purpose, stream): launches on different streams never share a workspace, so
    several batches can be in flight at once.  See workspace_scope for hipGraph capture."""
    key = (str(device), tag, _st())
    scoped = bool(_ws_scopes)
    store = _ws_scopes[-1] if scoped else _ws_cache
    ws = store.get(key)
    if ws is not None and ws.numel() >= nbytes:
        return ws
    new = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
    if scoped:
        if ws is not None:
            store.setdefault("_retired", []).append(ws)
        store[key] = new
    elif torch.cuda.is_current_stream_capturing():
        # captured outside a scope: never enters (or evicts from) the eager cache, and is never freed
        _ws_captured.append(new)
    else:
        store[key] = new
    return new


# plans of one Sinkhorn call: at most this many bytes per group of pairs (0 = one call for the whole batch)
sinkhorn_group_bytes = 135 << 20


def sinkhorn_match(dist: torch.Tensor, bin_score: torch.Tensor, iters: int, threshold: float,
                   m_lens=None, n_lens=None, want_p: bool = False, dual_softmax: bool = False, n_valid: Optional[int] = None):
    """dist [B, M, ldd] (first n_valid (default ldd) columns valid).  Returns dict with matches0/1 (int64),
    matching_scores0/1 and optionally the full assignment matrix 'p' [B, M+1, N+1].  Limits: M <= 8191 rows and
    N <= 4351 columns (the dust-bin row and column come on top); a larger problem raises PramHipError."""
    L = _lib.load()
    _chk(dist, "dist")
    assert dist.is_contiguous() and dist.dim() == 3
    B, M, ldd = dist.shape
    N = n_valid or ldd
    m0 = torch.empty(B, M, device=dist.device, dtype=_INT64)
    m1 = torch.empty(B, N, device=dist.device, dtype=_INT64)
    s0 = torch.empty(B, M, device=dist.device, dtype=torch.float32)
    s1 = torch.empty(B, N, device=dist.device, dtype=torch.float32)
    p = torch.zeros(B, M + 1, N + 1, device=dist.device, dtype=torch.float32) if want_p else None
    bs = bin_score.reshape(1).float()
    # The 20 iterations stream the whole [m + 1, n + 1] plan of every pair: a group of pairs whose plans fit the 256 MB infinity
    # cache together iterates out of it (35 us per pair and call instead of 67 from HBM, profiles/r02_sinkhorn_batch.txt), so a
    # large batch runs group after group — same kernels, every pair its own rows: results do not depend on the grouping.
    # Default (round 5, profiles/r05_sinkhorn_group_ab.txt): groups of <= 135 MB (8 pairs of 2049 x 2049: +0.7 % queries/s in three
    # alternations on one box), but only when a group still holds at least four pairs — at 4097 x 4097 (67 MB per pair) two-pair
    # groups double the call's 42 dependent launches for nothing (-0.8 %).
    per_pair = (M + 1) * ((N + 4) // 4 * 4) * 4
    group = B
    if sinkhorn_group_bytes > 0 and sinkhorn_group_bytes // max(per_pair, 1) >= 4:
        group = max(1, min(B, sinkhorn_group_bytes // max(per_pair, 1)))
    for b0 in range(0, B, group):
        b1 = min(B, b0 + group)
        nb = b1 - b0
        ws = _workspace(L.pram_sinkhorn_workspace_bytes(nb, M, N), dist.device, "sinkhorn")
        sl = lambda t: None if t is None else _p(t[b0:b1])
        if dual_softmax:
            rc = L.pram_dual_softmax_match_f32(_p(dist[b0:b1]), ldd, sl(m_lens), sl(n_lens), _p(bs), float(threshold), sl(p), N + 1,
                                               _p(m0[b0:b1]), _p(m1[b0:b1]), _p(s0[b0:b1]), _p(s1[b0:b1]), nb, M, N, _p(ws), _st())
        else:
            rc = L.pram_sinkhorn_match_f32(_p(dist[b0:b1]), ldd, sl(m_lens), sl(n_lens), _p(bs), int(iters), float(threshold), sl(p),
                                           N + 1, _p(m0[b0:b1]), _p(m1[b0:b1]), _p(s0[b0:b1]), _p(s1[b0:b1]), nb, M, N, _p(ws), _st())
        _lib.check(rc, "pram_sinkhorn_match_f32")
    out = {"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1}
    if want_p:
        out["p"] = p
    return out


def adagml_prune(logit, thr, n_min_tokens, lens_in, x, cos, sin, ind, want_conf=False, ld_logit: int = 1):
    """-> (x_out, cos_out, sin_out, ind_out, lens_out int32 [S], n_below int32 [S], conf or None).  ld_logit > 1: ``logit`` is the
    [S * T, ld_logit] output of the pooling head's padded last Linear and the logits are its column 0, read in place."""
    L = _lib.load()
    if ld_logit > 1:
        S, T = x.shape[0], x.shape[1]
        assert logit.is_contiguous() and logit.numel() == S * T * ld_logit
    else:
        S, T = logit.shape
    ldx = x.shape[-1]
    # rows at and beyond the new length of a set are never written — and never read: every consumer is ragged (lens)
    x_o, cos_o, sin_o, ind_o = torch.empty_like(x), torch.empty_like(cos), torch.empty_like(sin), _filled(tuple(ind.shape), ind.device, torch.int32)
    lens_o = torch.empty(S, device=x.device, dtype=torch.int32)
    n_below = torch.empty(S, device=x.device, dtype=torch.int32)
    conf = _filled((S, T), x.device) if want_conf else None
    row_map = torch.empty(S, T, device=x.device, dtype=torch.int32)
    _lib.check(L.pram_adagml_prune_ld_f32(_p(logit), int(ld_logit), float(thr), int(n_min_tokens), _p(lens_in), _p(x), _p(cos), _p(sin), _p(ind),
                                          _p(x_o), _p(cos_o), _p(sin_o), _p(ind_o), _p(lens_o), _p(n_below), _p(conf), _p(row_map),
                                          S, T, ldx, _st()),
               "pram_adagml_prune_f32")
    return x_o, cos_o, sin_o, ind_o, lens_o, n_below, conf


def adagml_scores4(col_self: torch.Tensor, col_cross: torch.Tensor) -> torch.Tensor:
    """[S, T] self / cross attention scores per token -> [S * T, 4] rows (self, cross, 0, 0): the pooling head's input."""
    L = _lib.load()
    assert col_self.is_contiguous() and col_cross.is_contiguous() and col_self.shape == col_cross.shape
    out = torch.empty(col_self.numel(), 4, device=col_self.device, dtype=torch.float32)
    _lib.check(L.pram_adagml_scores4_f32(_p(col_self), _p(col_cross), _p(out), col_self.numel(), _st()), "pram_adagml_scores4_f32")
    return out


def adagml_layer_state(active, lens, lens_new, n_below, num_points, tiny, stop_layer, lens_final, ind, ind_final, pairs: int, t_max: int,
                       layer: int, last: bool):
    """One layer of the batched AdaGML bookkeeping (pram_adagml_layer_state) -> (active', lens', lens_stop, lens_eff); tiny,
    stop_layer, lens_final and ind_final are updated in place."""
    L = _lib.load()
    dev = lens.device
    active_o = torch.empty_like(active)
    lens_o = torch.empty_like(lens)
    lens_stop = torch.empty_like(lens)
    lens_eff = torch.empty_like(lens)
    _lib.check(L.pram_adagml_layer_state(_p(active), _p(active_o), _p(lens), _p(lens_o), _p(lens_new), _p(n_below), _p(num_points), _p(tiny),
                                         _p(stop_layer), _p(lens_final), _p(lens_stop), _p(lens_eff), _p(ind), _p(ind_final), int(pairs),
                                         int(t_max), int(layer), int(bool(last)), _st()), "pram_adagml_layer_state")
    return active_o, lens_o, lens_stop, lens_eff


def adagml_scatter(matches0, mscores0, ind0, ind1, lens0, m_full):
    L = _lib.load()
    B, T = matches0.shape
    out_m = _filled((B, m_full, 2), matches0.device, torch.int32, -1).view(_INT64).view(B, m_full)      # int64 -1 = two 0xFFFFFFFF words
    out_s = _filled((B, m_full), matches0.device)
    _lib.check(L.pram_adagml_scatter_f32(_p(matches0), _p(mscores0), _p(ind0), _p(ind1), _p(lens0), B, T, m_full, _p(out_m),
                                         _p(out_s), _st()), "pram_adagml_scatter_f32")
    return out_m, out_s


# ------------------------------------------------------------------------------------- SFD2
def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, bias=None, scale=None, shift=None, residual=None, ks: int = 3,
                stride: int = 1, relu: bool = False, precision: Optional[str] = None, l2norm: bool = False) -> torch.Tensor:
    """x [B,H,W,Cin] contiguous NHWC; w [Cout,ks,ks,Cin].  precision: see linear() (conv1a's 4-channel input always runs
    on the exact-fp32 kernel).  l2norm: F.normalize over the channels of every output pixel behind the layer — inside the
    convolution's epilogue on the split-fp16 path when Cout <= 128, as a second kernel (l2norm_rows_) otherwise."""
    L = _lib.load()
    _chk(x, "x")
    assert x.is_contiguous() and w.is_contiguous()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    out = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=torch.float32)
    prec = _check_precision(_tl("forced") or precision or gemm_prec())
    if prec == "x3" and Cin % 32 == 0:
        wh, wl, ws = split_weight(w)
        if l2norm and Cout <= 128 and FUSED_L2NORM:
            _lib.check(L.pram_conv2d_nhwc_x3_l2norm_f32(_p(x), B, H, W, Cin, _p(wh), _p(wl), ws, _p(bias), _p(scale), _p(shift), _p(residual),
                                                        _p(out), Cout, ks, stride, int(relu), _st()), "pram_conv2d_nhwc_x3_l2norm_f32")
            return out
        _lib.check(L.pram_conv2d_nhwc_x3_f32(_p(x), B, H, W, Cin, _p(wh), _p(wl), ws, _p(bias), _p(scale), _p(shift), _p(residual),
                                             _p(out), Cout, ks, stride, int(relu), _st()), "pram_conv2d_nhwc_x3_f32")
    elif prec == "f16" and Cin % 64 == 0:
        _lib.check(L.pram_conv2d_nhwc_f16_f32(_p(x), B, H, W, Cin, _p(_w16(w)), _p(bias), _p(scale), _p(shift), _p(residual),
                                              _p(out), Cout, ks, stride, int(relu), _st()), "pram_conv2d_nhwc_f16_f32")
    else:
        _lib.check(L.pram_conv2d_nhwc_f32(_p(x), B, H, W, Cin, _p(w), _p(bias), _p(scale), _p(shift), _p(residual), _p(out),
                                          Cout, ks, stride, int(relu), _st()), "pram_conv2d_nhwc_f32")
    return l2norm_rows_(out) if l2norm else out


# split-fp16 path, always on in the product: False routes to the two-kernel / vector-ALU form, which the tests use as the reference
FUSED_L2NORM = True      # F.normalize inside the producing convolution (False: a second kernel, l2norm_rows_)
GROUPED_X3 = True      # the grouped 3x3 on the matrix pipe (False: vector ALU)


def conv3x3_grouped_nhwc(x: torch.Tensor, w: torch.Tensor, scale, shift, groups: int, relu: bool) -> torch.Tensor:
    """Grouped 3x3 (8 channels per group) of the ResBlock, exact fp32 on the vector ALU."""
    L = _lib.load()
    assert x.is_contiguous() and w.is_contiguous()
    B, H, W, Cc = x.shape
    out = torch.empty_like(x)
    _lib.check(L.pram_conv3x3_grouped_nhwc_f32(_p(x), B, H, W, Cc, _p(w), _p(scale), _p(shift), _p(out), groups, int(relu), _st()),
               "pram_conv3x3_grouped_nhwc_f32")
    return out


def conv2d_nhwc_planes(x: torch.Tensor, w: torch.Tensor, bias=None, scale=None, shift=None, residual=None, ks: int = 1,
                       stride: int = 1, relu: bool = False):
    """conv2d_nhwc on the split-fp16 path with the result as fp16 planes (hi, lo), hi + lo = 16 y: the split operand of the next
    split-fp16 layer (conv3x3_grouped_planes), written once by the producer instead of being recomputed by the consumer."""
    L = _lib.load()
    _chk(x, "x")
    assert x.is_contiguous() and w.is_contiguous()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    hi = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=torch.float16)
    lo = torch.empty_like(hi)
    wh, wl, ws = split_weight(w)
    _lib.check(L.pram_conv2d_nhwc_x3_planes(_p(x), B, H, W, Cin, _p(wh), _p(wl), ws, _p(bias), _p(scale), _p(shift), _p(residual),
                                            _p(hi), _p(lo), Cout, ks, stride, int(relu), _st()), "pram_conv2d_nhwc_x3_planes")
    return hi, lo


def conv3x3_grouped_planes(hi: torch.Tensor, lo: torch.Tensor, w: torch.Tensor, scale, shift, groups: int, relu: bool) -> torch.Tensor:
    """Grouped 3x3 (8 channels per group) on the matrix pipe (pram_conv3x3_grouped_planes_x3_f32): (hi, lo) from
    conv2d_nhwc_planes, w [C, 3, 3, 8] fp32; fp32 NHWC result."""
    L = _lib.load()
    assert hi.is_contiguous() and lo.is_contiguous() and w.is_contiguous() and hi.dtype == lo.dtype == torch.float16
    B, H, W, Cc = hi.shape
    out = torch.empty(B, H, W, Cc, device=hi.device, dtype=torch.float32)
    wh, wl, ws = split_weight(w)
    _lib.check(L.pram_conv3x3_grouped_planes_x3_f32(_p(hi), _p(lo), B, H, W, Cc, _p(wh), _p(wl), ws, _p(scale), _p(shift), _p(out),
                                                    groups, int(relu), _st()), "pram_conv3x3_grouped_planes_x3_f32")
    return out


def sfd2_conv1(x4: torch.Tensor, wa: torch.Tensor, ba, sa, ta, wb: torch.Tensor, bb, sb, tb) -> torch.Tensor:
    """SFD2's conv1a -> conv1b (3x3 / stride 1 / 3 -> 64, then 3x3 / stride 2 / 64 -> 64, each bias -> BN -> ReLU; nets/sfd2.py:135-139,
    281-282) in ONE launch on the split-fp16 path (pram_sfd2_conv1_x3_f32): the 1.26 GB conv1a map never exists.  x4: the NHWC4 image
    (image_to_nhwc4) or the fp32 NCHW image [B, 3, H, W] itself; wa [64, 3, 3, 4], wb [64, 3, 3, 64] as conv2d_nhwc takes them.
    -> [B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64]."""
    L = _lib.load()
    assert x4.is_contiguous() and x4.dtype == torch.float32 and tuple(wa.shape) == (64, 3, 3, 4) and tuple(wb.shape) == (64, 3, 3, 64)
    nchw3 = x4.shape[-1] != 4
    if nchw3:
        assert x4.dim() == 4 and x4.shape[1] == 3
        B, _, H, W = x4.shape
    else:
        B, H, W, _ = x4.shape

    def pad48(t):      # [64][36] -> [64][48]: K padded to three 16-deep steps, then the usual split
        flat = t.reshape(64, 36).float()
        return split_weight_raw(torch.cat([flat, flat.new_zeros(64, 12)], 1).contiguous())
    _x3_status(x4.device)
    _mark_x3(x4.device)
    wah, wal, wsa = _derived(wa, "x3pad48", pad48)
    wbh, wbl, wsb = split_weight(wb)
    out = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64, device=x4.device, dtype=torch.float32)
    _lib.check(L.pram_sfd2_conv1_x3_f32(_p(x4), B, H, W, _p(wah), _p(wal), wsa, _p(ba), _p(sa), _p(ta), _p(wbh), _p(wbl), wsb,
                                        _p(bb), _p(sb), _p(tb), _p(out), int(nchw3), _st()), "pram_sfd2_conv1_x3_f32")
    return out


def image_to_nhwc4(img: torch.Tensor) -> torch.Tensor:
    L = _lib.load()
    img = img.contiguous()
    _chk(img, "image")
    B, Cc, H, W = img.shape
    assert Cc == 3
    out = torch.empty(B, H, W, 4, device=img.device, dtype=torch.float32)
    _lib.check(L.pram_image_to_nhwc4_f32(_p(img), _p(out), B, H, W, _st()), "pram_image_to_nhwc4_f32")
    return out


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    L = _lib.load()
    assert x.is_contiguous()
    B, H, W, Cc = x.shape
    out = torch.empty(B, Cc, H, W, device=x.device, dtype=torch.float32)
    _lib.check(L.pram_nhwc_to_nchw_f32(_p(x), _p(out), B, H, W, Cc, _st()), "pram_nhwc_to_nchw_f32")
    return out


def score_map(logits_nhwc: torch.Tensor) -> torch.Tensor:
    L = _lib.load()
    assert logits_nhwc.is_contiguous() and logits_nhwc.shape[-1] == 65
    B, Hc, Wc, _ = logits_nhwc.shape
    out = torch.empty(B, Hc * 8, Wc * 8, device=logits_nhwc.device, dtype=torch.float32)
    _lib.check(L.pram_score_map_f32(_p(logits_nhwc), _p(out), B, Hc, Wc, _st()), "pram_score_map_f32")
    return out


def simple_nms(score: torch.Tensor, radius: int) -> torch.Tensor:
    L = _lib.load()
    score = score.contiguous()
    _chk(score, "score")
    B, H, W = score.shape
    out = torch.empty_like(score)
    ws = _workspace(L.pram_simple_nms_workspace_bytes(B, H, W), score.device, "nms")
    _lib.check(L.pram_simple_nms_f32(_p(score), _p(out), B, H, W, int(radius), _p(ws), _st()), "pram_simple_nms_f32")
    return out


def select_keypoints(nms: torch.Tensor, conf_th: float, min_keypoints: int, border: int, max_keypoints: int,
                     fallback_ref: int = 0):
    """-> kpts [B,k,2] (x,y), scores [B,k], counts [B] int32 (device)."""
    L = _lib.load()
    assert nms.is_contiguous()
    B, H, W = nms.shape
    k = int(max_keypoints)
    ws = _workspace(L.pram_select_keypoints_workspace_bytes(B, H, W, k), nms.device, "select")
    kpts = _filled((B, k, 2), nms.device)
    scores = _filled((B, k), nms.device)
    counts = _filled((B,), nms.device, torch.int32)
    _lib.check(L.pram_select_keypoints_f32(_p(nms), B, H, W, float(conf_th), int(min_keypoints), int(border), k,
                                           int(fallback_ref), _p(kpts), _p(scores), _p(counts), _p(ws), _st()),
               "pram_select_keypoints_f32")
    return kpts, scores, counts


def sample_nhwc(fmap: torch.Tensor, kpts: torch.Tensor, lens: Optional[torch.Tensor], s: int, l2norm: bool) -> torch.Tensor:
    """fmap [B,fh,fw,C] NHWC, kpts [B,N,2] -> [B,N,C]"""
    L = _lib.load()
    assert fmap.is_contiguous()
    kpts = kpts.contiguous()
    B, fh, fw, Cc = fmap.shape
    N = kpts.shape[1]
    out = _filled((B, N, Cc), fmap.device)
    _lib.check(L.pram_sample_nhwc_f32(_p(fmap), B, fh, fw, Cc, _p(kpts), _p(lens), N, int(s), int(l2norm), _p(out), _st()),
               "pram_sample_nhwc_f32")
    return out


# The descriptor head at the sampled pixels only (sparse_descriptors): taken when the row list is shorter than this fraction of the
# map.  Measured back to back on 16 frames of 120 x 160 (profiles/r07_sparse_desc_head.txt): the dense chain takes 1245 us whatever
# k is; the list chain 552 / 818 / 1067 us at k = 2048 / 3072 / 4096 (lists of 0.427 / 0.640 / 0.853 of the map), i.e. 45 us +
# 62 us per 1024 listed rows, which meets the dense chain at a list of about the whole map.  0.9 keeps the largest list that was
# measured (0.853: 14 % faster, the spread is 0.5 %) and nothing beyond it.
SPARSE_DESC_MAX_FRACTION = 0.9
SPARSE_ROWS_TILE = 256      # rows of a tile of the row-list chain (conv.hip ROWS_BM)


def sparse_desc_rows(n_max: int, fh: int, fw: int) -> int:
    """Rows per frame of the row-list chain for n_max keypoints on an fh x fw map, or 0 where the dense head is to be used."""
    r = -(-min(4 * n_max, fh * fw) // SPARSE_ROWS_TILE) * SPARSE_ROWS_TILE
    return r if 0 < r < SPARSE_DESC_MAX_FRACTION * fh * fw and fh * fw <= (1 << 18) else 0


def sparse_descriptors(x: torch.Tensor, w3: torch.Tensor, b3, w1: torch.Tensor, b1, kpts: torch.Tensor, lens: Optional[torch.Tensor],
                       s: int, rlen: int, want_parts: bool = False):
    """sample_nhwc(conv2d_nhwc(conv2d_nhwc(x, w3, b3, ks=3), w1, b1, ks=1, l2norm=True), kpts, lens, s, True), bit for bit, with the
    two convolutions computed only at the map pixels the keypoints sample (split-fp16 path; x [B,fh,fw,Cin] NHWC, w3 [C,3,3,Cin],
    w1 [Cout<=128,1,1,C], kpts [B,N,2]).  rlen: rows per frame (sparse_desc_rows).  No host synchronisation.
    want_parts: also return (rows, n_rows, pix2row)."""
    L = _lib.load()
    _chk(x, "x")
    assert x.is_contiguous() and w3.is_contiguous() and w1.is_contiguous()
    kpts = kpts.contiguous()
    B, fh, fw, Cin = x.shape
    N = kpts.shape[1]
    Cm, Cout = w3.shape[0], w1.shape[0]
    dev = x.device
    rows = torch.empty(B, rlen, device=dev, dtype=torch.int32)
    n_rows = torch.empty(B, device=dev, dtype=torch.int32)
    pix2row = torch.empty(B, fh * fw, device=dev, dtype=torch.int32)
    _lib.check(L.pram_sfd2_row_list(_p(kpts), _p(lens), B, N, fh, fw, int(s), _p(rows), _p(n_rows), _p(pix2row), rlen, _st()),
               "pram_sfd2_row_list")
    mid = torch.empty(B * rlen, Cm, device=dev, dtype=torch.float32)
    wh, wl, ws = split_weight(w3)
    _lib.check(L.pram_conv3x3_rows_x3_f32(_p(x), B, fh, fw, Cin, _p(wh), _p(wl), ws, _p(b3), _p(rows), _p(n_rows), rlen, _p(mid), Cm, 0,
                                          _st()), "pram_conv3x3_rows_x3_f32")
    dmat = torch.empty(B * rlen, Cout, device=dev, dtype=torch.float32)
    wh, wl, ws = split_weight(w1)
    _lib.check(L.pram_conv1x1_rows_x3_l2norm_f32(_p(mid), B, rlen, Cm, _p(wh), _p(wl), ws, _p(b1), _p(n_rows), _p(dmat), Cout, _st()),
               "pram_conv1x1_rows_x3_l2norm_f32")
    out = _filled((B, N, Cout), dev)
    _lib.check(L.pram_sample_rows_f32(_p(dmat), _p(pix2row), B, rlen, fh, fw, Cout, _p(kpts), _p(lens), N, int(s), 1, _p(out), _st()),
               "pram_sample_rows_f32")
    return (out, rows, n_rows, pix2row) if want_parts else out


def sampled_descriptors(x: torch.Tensor, w3: torch.Tensor, b3, w1: torch.Tensor, b1, kpts: torch.Tensor, lens: Optional[torch.Tensor],
                        s: int) -> torch.Tensor:
    """The descriptor head behind its first layer for a caller that wants the keypoints' descriptors and not the map:
    sparse_descriptors where the pixel list is short enough to pay (sparse_desc_rows), the dense layers and sample_nhwc
    otherwise — the same bits either way.  Split-fp16 path only."""
    rlen = sparse_desc_rows(kpts.shape[1], x.shape[1], x.shape[2]) if FUSED_L2NORM else 0
    if rlen:
        return sparse_descriptors(x, w3, b3, w1, b1, kpts, lens, s, rlen)
    dm = conv2d_nhwc(conv2d_nhwc(x, w3, b3, ks=3, precision="x3"), w1, b1, ks=1, precision="x3", l2norm=True)
    return sample_nhwc(dm, kpts, lens, s, True)


def l2norm_rows_(x: torch.Tensor) -> torch.Tensor:
    L = _lib.load()
    assert x.is_contiguous()
    cols = x.shape[-1]
    _lib.check(L.pram_l2norm_rows_f32(_p(x), x.numel() // cols, cols, _st()), "pram_l2norm_rows_f32")
    return x


def score_lookup(score_map_: torch.Tensor, kpts: torch.Tensor, lens: Optional[torch.Tensor]) -> torch.Tensor:
    L = _lib.load()
    score_map_ = score_map_.contiguous()
    kpts = kpts.contiguous()
    B, H, W = score_map_.shape
    Bk, N = kpts.shape[0], kpts.shape[1]
    out = _filled((Bk, N), kpts.device)
    stride = 0 if B == 1 else H * W
    _lib.check(L.pram_score_lookup_f32(_p(score_map_), stride, H, W, _p(kpts), _p(lens), Bk, N, _p(out), _st()),
               "pram_score_lookup_f32")
    return out


# ------------------------------------------------------------------------------------- edges of the path
def resize_bilinear(x: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """F.interpolate(x, size=(oh, ow), mode='bilinear', align_corners=True) for [..., h, w] planar maps."""
    L = _lib.load()
    x = x.contiguous().float()
    _chk(x, "x")
    h, w = x.shape[-2:]
    planes = x.numel() // (h * w)
    out = torch.empty(*x.shape[:-2], oh, ow, device=x.device, dtype=torch.float32)
    _lib.check(L.pram_resize_bilinear_f32(_p(x), _p(out), planes, h, w, int(oh), int(ow), _st()), "pram_resize_bilinear_f32")
    return out


def seg_epilogue(logits: torch.Tensor, lens: Optional[torch.Tensor], bg_threshold: float, want_scores: bool = False):
    """logits [B,N,C] -> seg_ids int32 [B,N], non_bg_mask int32 [B,N], n_non_bg int32 [B], seg_scores or None."""
    L = _lib.load()
    logits = logits.contiguous()
    _chk(logits, "logits")
    B, N, Cc = logits.shape
    ids = _filled((B, N), logits.device, torch.int32, -2)
    mask = _filled((B, N), logits.device, torch.int32)
    cnt = torch.empty(B, device=logits.device, dtype=torch.int32)      # cleared by the entry itself
    sc = _filled(tuple(logits.shape), logits.device) if want_scores else None
    _lib.check(L.pram_seg_epilogue_f32(_p(logits), _p(lens), B, N, Cc, float(bg_threshold), _p(sc), _p(ids), _p(mask), _p(cnt), _st()),
               "pram_seg_epilogue_f32")
    return ids, mask, cnt, sc


def row_sort_desc(x: torch.Tensor):
    L = _lib.load()
    x = x.contiguous()
    rows, cols = _rows2d(x, "x")
    vals = torch.empty_like(x)
    idx = torch.empty(x.shape, device=x.device, dtype=_INT64)
    _lib.check(L.pram_row_sort_desc_f32(_p(x), cols, rows, cols, _p(vals), _p(idx), _st()), "pram_row_sort_desc_f32")
    return vals, idx


def row_top2(x: torch.Tensor, largest: bool, n_valid: Optional[int] = None, row_lens=None, col_lens=None):
    """x [B,M,ld] -> (best [B,M], second [B,M], index of best int64 [B,M])"""
    L = _lib.load()
    assert x.is_contiguous() and x.dim() == 3
    B, M, ld = x.shape
    N = n_valid or ld
    v0 = torch.zeros(B, M, device=x.device, dtype=torch.float32)
    v1 = torch.zeros(B, M, device=x.device, dtype=torch.float32)
    i0 = torch.full((B, M), -1, device=x.device, dtype=_INT64)
    _lib.check(L.pram_row_top2_f32(_p(x), ld, M * ld, _p(row_lens), _p(col_lens), B, M, N, int(largest), _p(v0), _p(v1), _p(i0), _st()),
               "pram_row_top2_f32")
    return v0, v1, i0


def proj_dist_top2(sim: torch.Tensor, kpts: torch.Tensor, proj_uv: torch.Tensor, rng: float, n_valid: Optional[int] = None):
    """sim [M, ld] fp32, kpts [M,2], proj_uv [2,N] -> (d0 [M], d1 [M], i0 int64 [M])"""
    L = _lib.load()
    assert sim.is_contiguous() and sim.dim() == 2
    M, ld = sim.shape
    N = n_valid or ld
    kpts, proj_uv = kpts.contiguous().float(), proj_uv.contiguous().float()
    d0 = torch.zeros(M, device=sim.device, dtype=torch.float32)
    d1 = torch.zeros(M, device=sim.device, dtype=torch.float32)
    i0 = torch.full((M,), -1, device=sim.device, dtype=_INT64)
    _lib.check(L.pram_proj_dist_top2_f32(_p(sim), ld, _p(kpts), _p(proj_uv), M, N, float(rng), _p(d0), _p(d1), _p(i0), _st()),
               "pram_proj_dist_top2_f32")
    return d0, d1, i0


def proj_dist_top2_f64uv(sim: torch.Tensor, kpts: torch.Tensor, proj_uv: torch.Tensor, rng: float, n_valid: int):
    """proj_dist_top2 with float64 projections [2, ldu] (first n_valid columns valid): the pixel error and its `>= rng` test
    are float64, as in the reference (float32 keypoints - float64 projections)."""
    L = _lib.load()
    assert sim.is_contiguous() and sim.dim() == 2 and proj_uv.dtype == torch.float64 and proj_uv.is_contiguous() and proj_uv.dim() == 2
    M, ld = sim.shape
    kpts = kpts.contiguous().float()
    d0 = torch.zeros(M, device=sim.device, dtype=torch.float32)
    d1 = torch.zeros(M, device=sim.device, dtype=torch.float32)
    i0 = torch.full((M,), -1, device=sim.device, dtype=_INT64)
    _lib.check(L.pram_proj_dist_top2_f64uv(_p(sim), ld, _p(kpts), _p(proj_uv), proj_uv.shape[1], M, int(n_valid), float(rng), _p(d0), _p(d1),
                                           _p(i0), _st()), "pram_proj_dist_top2_f64uv")
    return d0, d1, i0


def project_points(xyz: torch.Tensor, K: torch.Tensor, Tcw: torch.Tensor, im_w: float, im_h: float):
    """xyz [N,3], K [3,3], Tcw [4,4] float64 on the device -> (uvd [3,N] f64, mask int32 [N], keep_idx int32 [N], uv_keep f64 [2,N],
    count int32 [1]) — projection, frustum test and ordered compaction of singlemap3d.py:405-415; nothing synchronises."""
    L = _lib.load()
    for t, nm in ((xyz, "xyz"), (K, "K"), (Tcw, "Tcw")):
        _chk(t, nm, torch.float64)
    xyz, K, Tcw = xyz.contiguous(), K.contiguous(), Tcw.contiguous()
    n = xyz.shape[0]
    dev = xyz.device
    uvd = torch.empty(3, n, device=dev, dtype=torch.float64)
    mask = torch.empty(n, device=dev, dtype=torch.int32)
    keep = torch.empty(n, device=dev, dtype=torch.int32)
    uvk = torch.empty(2, max(n, 1), device=dev, dtype=torch.float64)
    count = torch.zeros(1, device=dev, dtype=torch.int32)
    if n == 0:      # nothing to project: the empty outputs have no storage to hand to the entry
        return uvd, mask, keep, uvk, count
    _lib.check(L.pram_project_points_f64(_p(xyz), _p(K), _p(Tcw), n, float(im_w), float(im_h), _p(uvd), _p(mask), _p(keep), _p(uvk),
                                         _p(count), _st()), "pram_project_points_f64")
    return uvd, mask, keep, uvk, count


def seg_vote(sorted_vals: torch.Tensor, sorted_ids: torch.Tensor, topk: int):
    """Landmark vote over the sorted class lists of row_sort_desc ([N, C] each) -> device tensors
    (win_sid [topk], win_rank [topk], win_count [topk], n_win [1], tokens [topk, N], mean_score [topk])."""
    L = _lib.load()
    assert sorted_vals.is_contiguous() and sorted_ids.is_contiguous() and sorted_ids.dtype == _INT64
    n, c = sorted_vals.shape
    dev = sorted_vals.device
    sid = torch.zeros(topk, device=dev, dtype=torch.int32)
    rank = torch.zeros(topk, device=dev, dtype=torch.int32)
    cnt = torch.zeros(topk, device=dev, dtype=torch.int32)
    nwin = torch.zeros(1, device=dev, dtype=torch.int32)
    tokens = torch.zeros(topk, max(n, 1), device=dev, dtype=torch.int32)
    mean = torch.zeros(topk, device=dev, dtype=torch.float32)
    if n == 0:      # no tokens, no winners: the empty class lists have no storage to hand to the entry
        return sid, rank, cnt, nwin, tokens, mean
    _lib.check(L.pram_seg_vote(_p(sorted_ids), _p(sorted_vals), n, c, int(topk), _p(sid), _p(rank), _p(cnt), _p(nwin), _p(tokens), _p(mean),
                               _st()), "pram_seg_vote")
    return sid, rank, cnt, nwin, tokens, mean


def frame_lut(mean, std, device) -> torch.Tensor:
    """[3, 256] fp32: what the reference's frame preparation makes of byte v in channel c — `img / 255` in float64 (numpy),
    `.float()`, then tvf.Normalize's `sub_(mean).div_(std)` in fp32 (localization/loc_by_rec_online.py:98-106) — computed with exactly
    those operations, on the host."""
    v = (torch.arange(256, dtype=torch.float64) / 255).float()[None].repeat(3, 1)
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1)
    return v.sub_(m).div_(s).contiguous().to(device)


def stage_frames(frames_u8: torch.Tensor, lut: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B, H, W, 3] (cv2 layout, on the device) -> normalised fp32 [B, 3, H, W] (pram_stage_frames_u8): the device half of the
    reference's per-frame preparation; `lut` from frame_lut()."""
    L = _lib.load()
    _chk(frames_u8, "frames", torch.uint8)
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and frames_u8.dim() == 4 and frames_u8.shape[-1] == 3
    B, H, W, _ = frames_u8.shape
    if not (lut.is_cuda and lut.device == frames_u8.device and lut.dtype == torch.float32 and lut.is_contiguous() and tuple(lut.shape) == (3, 256)):
        raise _lib.PramHipError("stage_frames: lut must be the contiguous fp32 [3, 256] table of frame_lut() on the frames' device")
    if out is None:
        out = torch.empty(B, 3, H, W, device=frames_u8.device, dtype=torch.float32)
    if not (out.is_cuda and out.device == frames_u8.device and out.is_contiguous() and tuple(out.shape) == (B, 3, H, W) and out.dtype == torch.float32):
        raise _lib.PramHipError("stage_frames: out must be a contiguous fp32 [B, 3, H, W] tensor on the frames' device")
    _lib.check(L.pram_stage_frames_u8(_p(frames_u8), _p(lut), _p(out), B, H, W, _st()), "pram_stage_frames_u8")
    return out


def pack_record(kpts: torch.Tensor, scores: torch.Tensor, landmark: Optional[torch.Tensor] = None,
                matches0: Optional[torch.Tensor] = None, mscores0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> [B, k, 6] fp32: x, y, score, landmark id, match index, match score (pram_pack_record_f32); matches0 / mscores0 may cover
    only the first km <= k keypoints of every query."""
    L = _lib.load()
    kpts, scores = kpts.contiguous(), scores.contiguous()
    _chk(kpts, "kpts"), _chk(scores, "scores")
    B, k = scores.shape
    km = 0
    if matches0 is not None:
        matches0, mscores0 = matches0.contiguous(), mscores0.contiguous()
        assert matches0.dtype == _INT64 and mscores0.dtype == torch.float32 and matches0.shape == mscores0.shape
        km = matches0.shape[1]
    if landmark is not None:
        landmark = landmark.contiguous()
        assert landmark.dtype == torch.int32
    rec = torch.empty(B, k, 6, device=scores.device, dtype=torch.float32)
    _lib.check(L.pram_pack_record_f32(_p(kpts), _p(scores), _p(landmark), _p(matches0), _p(mscores0), B, k, km, _p(rec), _st()),
               "pram_pack_record_f32")
    return rec


# ---- candidate-landmark matching (csrc/candidates.hip; pram_amd/localization/candidates.py drives these) -------------------
CAND_PLAN_COLS = 10      # PRAM_CAND_PLAN_COLS
CAND_PLAN_FIELDS = ("query", "sid", "frame", "semantic", "lens0", "lens1", "tok_off", "row0", "sel_off", "order")


def seg_vote_batched(sorted_vals: torch.Tensor, sorted_ids: torch.Tensor, topk: int):
    """pram_seg_vote for a batch of queries ([B, N, C] sorted class lists): one launch per query into slices of batched buffers
    -> (win_sid [B, topk], win_rank, win_count, n_win [B], tokens [B, topk, N], mean_score [B, topk]), all on the device."""
    L = _lib.load()
    _chk(sorted_vals, "sorted_vals")
    _chk(sorted_ids, "sorted_ids", _INT64)
    assert sorted_vals.is_contiguous() and sorted_ids.is_contiguous() and sorted_vals.dim() == 3 and sorted_ids.shape == sorted_vals.shape
    B, n, c = sorted_vals.shape
    dev = sorted_vals.device
    topk = int(topk)
    sid, rank, cnt = _filled((B, topk), dev, torch.int32), _filled((B, topk), dev, torch.int32), _filled((B, topk), dev, torch.int32)
    nwin = _filled((B,), dev, torch.int32)
    tokens = _filled((B, topk, max(n, 1)), dev, torch.int32)
    mean = _filled((B, topk), dev)
    st = _st()
    for b in range(B if n else 0):      # n == 0: no tokens, no winners (the zero fill above)
        _lib.check(L.pram_seg_vote(_p(sorted_ids[b]), _p(sorted_vals[b]), n, c, topk, _p(sid[b]), _p(rank[b]), _p(cnt[b]), _p(nwin[b:]),
                                   _p(tokens[b]), _p(mean[b]), st), "pram_seg_vote")
    return sid, rank, cnt, nwin, tokens, mean


def cand_mask_ranks_(sorted_ids: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """In place: the sorted class ids [B, N, C] of the padded tokens (t >= counts[b]) become 0 (background) at every rank."""
    L = _lib.load()
    _chk(sorted_ids, "sorted_ids", _INT64)
    _chk(counts, "counts", torch.int32)
    assert sorted_ids.is_contiguous() and sorted_ids.dim() == 3 and counts.is_contiguous() and counts.numel() == sorted_ids.shape[0]
    B, n, c = sorted_ids.shape
    _lib.check(L.pram_cand_mask_ranks(_p(sorted_ids), _p(counts), B, n, c, _st()), "pram_cand_mask_ranks")
    return sorted_ids


def cand_plan(win_sid, win_count, n_win, seg_ids, counts, n_class: int, store, min_kpts: int, overlap_ratio: float,
              semantic_matching: bool) -> torch.Tensor:
    """-> plan int32 [CAND_PLAN_COLS, B * seg_k] (one contiguous column per CAND_PLAN_FIELDS entry).  ``store``: the device tables
    of a ReferenceStore (dict of tensors: pram_cand_plan) or of a MultiMapStore (they carry lm_start: pram_cand_plan_maps)."""
    L = _lib.load()
    for t, nm in ((win_sid, "win_sid"), (win_count, "win_count"), (n_win, "n_win"), (seg_ids, "seg_ids"), (counts, "counts")):
        _chk(t, nm, torch.int32)
        assert t.is_contiguous(), nm
    B, seg_k = win_sid.shape
    n = seg_ids.shape[1]
    assert seg_ids.shape[0] == B and counts.numel() == B and n_win.numel() == B and win_count.shape == win_sid.shape
    plan = torch.empty(CAND_PLAN_COLS, B * seg_k, device=win_sid.device, dtype=torch.int32)
    s = store
    if "lm_start" in s:      # a MultiMapStore's tables: the landmark tables are indexed by the global id
        _lib.check(L.pram_cand_plan_maps(_p(win_sid), _p(win_count), _p(n_win), _p(seg_ids), _p(counts), B, n, int(n_class), seg_k, _p(s["lm_frame"]),
                                         _p(s["lm_sel_off"]), _p(s["lm_sel_len"]), int(s["n_landmarks"]), _p(s["lm_start"]), _p(s["frame_off"]),
                                         _p(s["hist_off"]), _p(s["hist_label"]), _p(s["hist_cnt"]), int(s["n_frames"]), int(min_kpts),
                                         float(overlap_ratio), int(bool(semantic_matching)), _p(plan), _st()), "pram_cand_plan_maps")
        return plan
    _lib.check(L.pram_cand_plan(_p(win_sid), _p(win_count), _p(n_win), _p(seg_ids), _p(counts), B, n, int(n_class), seg_k, _p(s["lm_frame"]),
                                _p(s["lm_sel_off"]), _p(s["lm_sel_len"]), int(s["n_landmarks"]), int(s["start_sid"]), _p(s["frame_off"]),
                                _p(s["hist_off"]), _p(s["hist_label"]), _p(s["hist_cnt"]), int(s["n_frames"]), int(min_kpts),
                                float(overlap_ratio), int(bool(semantic_matching)), _p(plan), _st()), "pram_cand_plan")
    return plan


def cand_gather(plan: torch.Tensor, tokens: torch.Tensor, store, q_desc, q_kpts, q_scores, q_norm, t_pad: int):
    """-> dict(descriptors0/1 [P, T, 128], norm_keypoints0/1 [P, T, 2], scores0/1 [P, T]) filled from the plan; q_norm = (cx, cy, scale)
    of the queries' camera.  The two sides of each output are halves of one [2P, ...] buffer."""
    L = _lib.load()
    for t, nm in ((q_desc, "descriptors"), (q_kpts, "keypoints"), (q_scores, "scores")):
        _chk(t, nm)
        assert t.is_contiguous(), nm
    B, n, D = q_desc.shape
    assert D == 128 and tuple(q_kpts.shape) == (B, n, 2) and tuple(q_scores.shape) == (B, n)
    P, T, dev = plan.shape[1], int(t_pad), q_desc.device
    d = torch.empty(2 * P, T, 128, device=dev, dtype=torch.float32)
    k = torch.empty(2 * P, T, 2, device=dev, dtype=torch.float32)
    sc = torch.empty(2 * P, T, device=dev, dtype=torch.float32)
    s = store
    _lib.check(L.pram_cand_gather(_p(plan), _p(tokens), _p(s["sel_rows"]), _p(q_desc), _p(q_kpts), _p(q_scores), n, _p(s["descriptors"]),
                                  _p(s["keypoints"]), _p(s["scores"]), _p(s["frame_norm"]), int(s["n_rows"]), float(q_norm[0]), float(q_norm[1]),
                                  float(q_norm[2]), _p(d[:P]), _p(k[:P]), _p(sc[:P]), _p(d[P:]), _p(k[P:]), _p(sc[P:]), P, T, _st()),
               "pram_cand_gather")
    return {"descriptors0": d[:P], "descriptors1": d[P:], "norm_keypoints0": k[:P], "norm_keypoints1": k[P:], "scores0": sc[:P], "scores1": sc[P:]}


# The match list every stage hands on: parallel tensors [P, cap] + tail with count int32 [P].  Key -> (dtype, tail), in the order
# the entries of pram_hip.h take the pointers.
MATCH_LIST = {"matched_keypoint_ids": (_INT64, ()), "matched_keypoints": (torch.float32, (2,)), "matched_ref_keypoints": (torch.float32, (2,)),
              "matched_point3D_ids": (_INT64, ()), "matched_xyzs": (torch.float64, (3,)), "matched_sids": (torch.int32, ())}
MATCH_KEYS = tuple(MATCH_LIST)
MATCH_REF_KPTS, MATCH_SRC = "matched_ref_keypoints", "matched_src"      # the list projref_correspond leaves out, the one refine_merge adds
MATCH_NOREF_KEYS = tuple(k for k in MATCH_KEYS if k != MATCH_REF_KPTS)
MATCH_POINT_KEYS = tuple(k for k in MATCH_NOREF_KEYS if k != "matched_keypoints")      # the four lists update_point3ds reads
# the order the result dicts of localization/ list them in (the reference's)
MATCH_RESULT_KEYS = tuple(MATCH_KEYS[i] for i in (1, 0, 4, 3, 5, 2))


def _cor_chk(cor: dict, name: str, keys=MATCH_KEYS, src: bool = False):
    """dtypes, contiguity and shapes of the lists ``keys`` of cor (src: and of matched_src) and of its count -> (P, cap)."""
    P, t = cor["matched_keypoint_ids"].shape
    for k in keys + ((MATCH_SRC,) if src else ()):
        dt, tail = MATCH_LIST.get(k, (torch.int32, ()))
        _chk(cor[k], f"{name}.{k}", dt)
        assert cor[k].is_contiguous() and tuple(cor[k].shape) == (P, t) + tail, (name, k)
    _chk(cor["count"], f"{name}.count", torch.int32)
    assert cor["count"].is_contiguous() and cor["count"].numel() == P
    return P, t


def _cor_alloc(B: int, cap: int, dev, keys=MATCH_KEYS, src: bool = False) -> dict:
    """Uninitialised lists ``keys`` [B, max(cap, 1)] (src: and matched_src), then count."""
    c1 = max(int(cap), 1)
    out = {k: torch.empty((B, c1) + MATCH_LIST[k][1], device=dev, dtype=MATCH_LIST[k][0]) for k in keys}
    if src:
        out[MATCH_SRC] = torch.empty(B, c1, device=dev, dtype=torch.int32)
    out["count"] = torch.empty(B, device=dev, dtype=torch.int32)
    return out


def cand_correspond(matches0: torch.Tensor, plan: torch.Tensor, tokens: torch.Tensor, store, q_kpts: torch.Tensor, cap: int):
    """matches0 int64 [P, >= T0] -> dict of padded per-pair outputs [P, cap, ...] and count int32 [P] (pram_cand_correspond)."""
    L = _lib.load()
    _chk(matches0, "matches0", _INT64)
    _chk(q_kpts, "keypoints")
    assert matches0.dim() == 2 and matches0.stride(1) == 1 and q_kpts.is_contiguous()
    P, t0 = matches0.shape
    assert plan.shape[1] == P
    n, cap = q_kpts.shape[1], int(cap)
    out = _cor_alloc(P, cap, matches0.device)
    s = store
    _lib.check(L.pram_cand_correspond(_p(matches0), matches0.stride(0), _p(plan), _p(tokens), _p(s["sel_rows"]), _p(q_kpts), n, _p(s["keypoints"]),
                                      _p(s["xyzs"]), _p(s["point3D_ids"]), _p(s["keypoint_segs"]), int(s["n_rows"]), P, t0, cap,
                                      *[_p(out[k]) for k in MATCH_KEYS], _p(out["count"]), _st()), "pram_cand_correspond")
    return out


# ---- batched absolute pose (csrc/pose.hip; pram_amd/localization/pose.py drives these) ---------------------------------------
CAMERA_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4}      # PRAM_CAM_*
POSE_CAM_PARAMS = 8      # PRAM_POSE_CAM_PARAMS


def _pose_chk(m_kpts, m_xyz, counts):
    _chk(m_kpts, "matched_keypoints")
    _chk(m_xyz, "matched_xyzs", torch.float64)
    _chk(counts, "counts", torch.int32)
    assert m_kpts.is_contiguous() and m_xyz.is_contiguous() and counts.is_contiguous()
    P, t0 = m_kpts.shape[:2]
    assert tuple(m_kpts.shape) == (P, t0, 2) and tuple(m_xyz.shape) == (P, t0, 3) and counts.numel() == P
    return P, t0


def _pose_chk_stage(norm_pts, m_xyz, counts, cam_model, cam_params, seg_k):
    """dtype, device, contiguity and shapes of what pose_score / pose_refine hand over as raw pointers -> (P, t0, B)."""
    _chk(norm_pts, "norm_pts", torch.float64)
    _chk(m_xyz, "matched_xyzs", torch.float64)
    _chk(counts, "counts", torch.int32)
    _chk(cam_model, "cam_model", torch.int32)
    _chk(cam_params, "cam_params", torch.float64)
    assert norm_pts.is_contiguous() and m_xyz.is_contiguous() and counts.is_contiguous() and cam_model.is_contiguous() and cam_params.is_contiguous()
    P, t0 = norm_pts.shape[:2]
    B, seg_k = cam_model.numel(), int(seg_k)
    assert tuple(norm_pts.shape) == (P, t0, 2) and tuple(m_xyz.shape) == (P, t0, 3) and counts.numel() == P
    assert seg_k >= 1 and P == B * seg_k and tuple(cam_params.shape) == (B, POSE_CAM_PARAMS)
    return P, t0, B


def pose_prepare(m_kpts: torch.Tensor, counts: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor, cam_model_host,
                 seg_k: int) -> torch.Tensor:
    """matched_keypoints float32 [P, t0, 2] (+ 0.5 inside) -> normalised camera-plane points float64 [P, t0, 2]; rows >= counts[p]
    are left unwritten.  cam_model int32 [B], cam_params float64 [B, 8] on the device, cam_model_host: the ids on the host
    (a sequence of ints), which is what the launcher validates."""
    import ctypes
    L = _lib.load()
    _chk(m_kpts, "matched_keypoints")
    _chk(counts, "counts", torch.int32)
    _chk(cam_model, "cam_model", torch.int32)
    _chk(cam_params, "cam_params", torch.float64)
    assert m_kpts.is_contiguous() and counts.is_contiguous() and cam_model.is_contiguous() and cam_params.is_contiguous()
    P, t0 = m_kpts.shape[:2]
    B, seg_k = cam_model.numel(), int(seg_k)
    assert seg_k >= 1 and P == B * seg_k and counts.numel() == P and tuple(cam_params.shape) == (B, POSE_CAM_PARAMS) and len(cam_model_host) == B
    host = (ctypes.c_int * max(B, 1))(*[int(m) for m in cam_model_host])
    pts = torch.empty(P, t0, 2, device=m_kpts.device, dtype=torch.float64)
    _lib.check(L.pram_pose_prepare(_p(m_kpts), _p(counts), _p(cam_model), _p(cam_params), ctypes.addressof(host), B, seg_k, t0, _p(pts), _st()),
               "pram_pose_prepare")
    return pts


def pose_hypotheses(norm_pts: torch.Tensor, m_xyz: torch.Tensor, counts: torch.Tensor, trials: int, seed: int, with_triples: bool = False):
    """-> (poses float64 [P, trials, 4, 12], n_sol int32 [P, trials][, triples int32 [P, trials, 3]])."""
    L = _lib.load()
    _chk(norm_pts, "norm_pts", torch.float64)
    _chk(m_xyz, "matched_xyzs", torch.float64)
    _chk(counts, "counts", torch.int32)
    assert norm_pts.is_contiguous() and m_xyz.is_contiguous() and counts.is_contiguous()
    P, t0 = norm_pts.shape[:2]
    assert tuple(m_xyz.shape) == (P, t0, 3) and counts.numel() == P
    trials, dev = int(trials), norm_pts.device
    poses = torch.empty(P, max(trials, 1), 4, 12, device=dev, dtype=torch.float64)
    n_sol = torch.empty(P, max(trials, 1), device=dev, dtype=torch.int32)
    tri = torch.empty(P, max(trials, 1), 3, device=dev, dtype=torch.int32) if with_triples else None
    _lib.check(L.pram_pose_hypotheses(_p(norm_pts), _p(m_xyz), _p(counts), P, t0, trials, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(poses), _p(n_sol),
                                      _p(tri), _st()), "pram_pose_hypotheses")
    return (poses, n_sol, tri) if with_triples else (poses, n_sol)


def pose_score(norm_pts, m_xyz, counts, poses, n_sol, cam_model, cam_params, seg_k: int, threshold: float):
    """-> (h_inliers int32 [P, trials * 4] (-1 = empty slot), h_resid float64 [P, trials * 4], best int32 [P])."""
    L = _lib.load()
    P, t0, B = _pose_chk_stage(norm_pts, m_xyz, counts, cam_model, cam_params, seg_k)
    trials, dev = poses.shape[1], norm_pts.device
    _chk(poses, "poses", torch.float64)
    _chk(n_sol, "n_sol", torch.int32)
    assert poses.is_contiguous() and n_sol.is_contiguous() and tuple(poses.shape) == (P, trials, 4, 12) and tuple(n_sol.shape) == (P, trials)
    h_inl = torch.empty(P, trials * 4, device=dev, dtype=torch.int32)
    h_res = torch.empty(P, trials * 4, device=dev, dtype=torch.float64)
    best = torch.empty(P, device=dev, dtype=torch.int32)
    _lib.check(L.pram_pose_score(_p(norm_pts), _p(m_xyz), _p(counts), _p(poses), _p(n_sol), _p(cam_model), _p(cam_params), P, int(seg_k), t0, trials,
                                 float(threshold), _p(h_inl), _p(h_res), _p(best), _st()), "pram_pose_score")
    return h_inl, h_res, best


def pose_refine(m_kpts, norm_pts, m_xyz, counts, poses, h_inl, best, cam_model, cam_params, seg_k: int, threshold: float,
                min_inlier_ratio: float, refine_iters: int) -> dict:
    """-> dict(qvec float64 [P, 4] (w, x, y, z), tvec [P, 3], inliers uint8 [P, t0], num_inliers int32 [P], success int32 [P])."""
    L = _lib.load()
    P, t0 = _pose_chk(m_kpts, m_xyz, counts)
    _pose_chk_stage(norm_pts, m_xyz, counts, cam_model, cam_params, seg_k)
    trials, dev = poses.shape[1], m_kpts.device
    _chk(poses, "poses", torch.float64)
    _chk(h_inl, "h_inliers", torch.int32)
    _chk(best, "best", torch.int32)
    assert poses.is_contiguous() and h_inl.is_contiguous() and best.is_contiguous()
    assert tuple(poses.shape) == (P, trials, 4, 12) and tuple(h_inl.shape) == (P, trials * 4) and best.numel() == P
    out = {"qvec": torch.empty(P, 4, device=dev, dtype=torch.float64), "tvec": torch.empty(P, 3, device=dev, dtype=torch.float64),
           "inliers": torch.empty(P, t0, device=dev, dtype=torch.uint8), "num_inliers": torch.empty(P, device=dev, dtype=torch.int32),
           "success": torch.empty(P, device=dev, dtype=torch.int32)}
    _lib.check(L.pram_pose_refine(_p(m_kpts), _p(norm_pts), _p(m_xyz), _p(counts), _p(poses), _p(h_inl), _p(best), _p(cam_model), _p(cam_params), P,
                                  int(seg_k), t0, trials, float(threshold), float(min_inlier_ratio), int(refine_iters), _p(out["qvec"]),
                                  _p(out["tvec"]), _p(out["inliers"]), _p(out["num_inliers"]), _p(out["success"]), _st()), "pram_pose_refine")
    return out


def pose_select(success: torch.Tensor, num_inliers: torch.Tensor, seg_k: int, min_inliers: int) -> torch.Tensor:
    """success / num_inliers int32 [B * seg_k] -> int32 [B, 3]: kept candidate (-1 none), tracking status (1 / 0 / -1 none), order."""
    L = _lib.load()
    _chk(success, "success", torch.int32)
    _chk(num_inliers, "num_inliers", torch.int32)
    seg_k = int(seg_k)
    assert success.is_contiguous() and num_inliers.is_contiguous() and success.numel() == num_inliers.numel()
    assert seg_k >= 1 and success.numel() % seg_k == 0
    B = success.numel() // seg_k
    chosen = torch.empty(B, 3, device=success.device, dtype=torch.int32)
    _lib.check(L.pram_pose_select(_p(success), _p(num_inliers), B, seg_k, int(min_inliers), _p(chosen), _st()), "pram_pose_select")
    return chosen


# ---- pose refinement by matching over covisible frames (csrc/refine.hip; pram_amd/localization/refine.py drives these) ---------
def refine_plan(chosen: torch.Tensor, loc_plan: torch.Tensor, counts: torch.Tensor, store, n_cov: int, enable: Optional[torch.Tensor] = None):
    """chosen int32 [B, 3] (pose_select), loc_plan int32 [CAND_PLAN_COLS, B * seg_k], counts int32 [B], ``store``: the device tables
    of a ReferenceStore -> (plan int32 [CAND_PLAN_COLS, B * n_cov], ref_frame, n_cov_used, init_on int32 [B])."""
    L = _lib.load()
    for t, nm in ((chosen, "chosen"), (loc_plan, "plan"), (counts, "counts")) + (((enable, "enable"),) if enable is not None else ()):
        _chk(t, nm, torch.int32)
        assert t.is_contiguous(), nm
    B, n_cov = counts.numel(), int(n_cov)
    assert tuple(chosen.shape) == (B, 3) and loc_plan.dim() == 2 and loc_plan.shape[0] == CAND_PLAN_COLS and (enable is None or enable.numel() == B)
    seg_k = loc_plan.shape[1] // B if B else 1
    assert seg_k >= 1 and loc_plan.shape[1] == B * seg_k
    dev = counts.device
    plan = torch.empty(CAND_PLAN_COLS, B * max(n_cov, 0), device=dev, dtype=torch.int32)
    ref_frame, used, init_on = (torch.empty(B, device=dev, dtype=torch.int32) for _ in range(3))
    s = store
    _lib.check(L.pram_refine_plan(_p(chosen), _p(loc_plan), _p(counts), _p(enable), _p(s["frame_off"]), _p(s["covis_off"]), _p(s["covis_frames"]),
                                  B, seg_k, n_cov, int(s["n_frames"]), int(s["n_covis"]), _p(plan), _p(ref_frame), _p(used), _p(init_on), _st()),
               "pram_refine_plan")
    return plan, ref_frame, used, init_on


def refine_merge(cor_ref: dict, cor_loc: dict, chosen: torch.Tensor, init_on: torch.Tensor, n_cov: int, out: Optional[dict] = None) -> dict:
    """cor_ref / cor_loc: cand_correspond's dicts for the B * n_cov refinement pairs and the B * seg_k localisation pairs
    -> one list per query, dict of [B, cap, ...] tensors (cap = n_cov * t0 + t0a) with the keys of cand_correspond plus
    matched_src int32 and count int32 [B].  ``out``: buffers to write into (the tests pre-fill them)."""
    L = _lib.load()
    Pr, t0 = _cor_chk(cor_ref, "refinement")
    Pa, t0a = _cor_chk(cor_loc, "localisation")
    _chk(chosen, "chosen", torch.int32)
    _chk(init_on, "init_on", torch.int32)
    B, n_cov = init_on.numel(), int(n_cov)
    assert chosen.is_contiguous() and init_on.is_contiguous() and tuple(chosen.shape) == (B, 3) and Pr == B * n_cov
    seg_k = Pa // B if B else 1
    assert seg_k >= 1 and Pa == B * seg_k
    if out is None:
        out = _cor_alloc(B, n_cov * t0 + t0a, init_on.device, src=True)
    else:
        assert _cor_chk(out, "out", src=True)[0] == B
    cap = out["matched_sids"].shape[1]
    r, a, o = cor_ref, cor_loc, out
    _lib.check(L.pram_refine_merge(*[_p(r[k]) for k in MATCH_KEYS], _p(r["count"]), t0, *[_p(a[k]) for k in MATCH_KEYS], _p(a["count"]), t0a,
                                   _p(chosen), _p(init_on), B, seg_k, n_cov, cap, *[_p(o[k]) for k in MATCH_KEYS], _p(o[MATCH_SRC]),
                                   _p(o["count"]), _st()), "pram_refine_merge")
    return out


def refine_frame_vote(m_point3d_ids: torch.Tensor, m_count: torch.Tensor, inliers: torch.Tensor, success: torch.Tensor, store, k: int):
    """find_reference_frames per query over the merged list -> (best_frames int32 [B, k] (store frame indices, -1 padded),
    best_counts int32 [B, k], n_best int32 [B])."""
    L = _lib.load()
    _chk(m_point3d_ids, "matched_point3D_ids", _INT64)
    _chk(m_count, "count", torch.int32)
    _chk(inliers, "inliers", torch.uint8)
    _chk(success, "success", torch.int32)
    B, cap = m_point3d_ids.shape
    assert m_point3d_ids.is_contiguous() and m_count.is_contiguous() and inliers.is_contiguous() and success.is_contiguous()
    assert tuple(inliers.shape) == (B, cap) and m_count.numel() == B and success.numel() == B
    dev, k, s = m_point3d_ids.device, int(k), store
    hist = torch.empty(B, max(int(s["n_frames"]), 1), device=dev, dtype=torch.int32)      # zeroed by the entry
    best_f, best_c = torch.empty(B, max(k, 1), device=dev, dtype=torch.int32), torch.empty(B, max(k, 1), device=dev, dtype=torch.int32)
    n_best = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.check(L.pram_refine_frame_vote(_p(m_point3d_ids), _p(m_count), _p(inliers), _p(success), B, cap, _p(s["pt_ids"]), _p(s["pt_off"]),
                                        _p(s["pt_frames"]), int(s["n_points"]), int(s["n_pt_entries"]), _p(s["is_vrf"]), int(s["n_frames"]), k,
                                        _p(hist), _p(best_f), _p(best_c), _p(n_best), _st()), "pram_refine_frame_vote")
    return best_f, best_c, n_best


# ---- pose refinement by projection over covisible frames (csrc/projref.hip; pram_amd/localization/refine.py drives these) ------
def projref_mark(chosen: torch.Tensor, loc_plan: torch.Tensor, store, n_cov: int, enable: Optional[torch.Tensor] = None):
    """chosen int32 [B, 3], loc_plan int32 [CAND_PLAN_COLS, B * seg_k], ``store``: the device tables of a ReferenceStore
    -> (bitmap int32 [B, ceil(n_points / 32)] over the point table, ref_frame int32 [B])."""
    L = _lib.load()
    for t, nm in ((chosen, "chosen"), (loc_plan, "plan")) + (((enable, "enable"),) if enable is not None else ()):
        _chk(t, nm, torch.int32)
        assert t.is_contiguous(), nm
    B, n_cov, s = chosen.shape[0], int(n_cov), store
    assert tuple(chosen.shape) == (B, 3) and loc_plan.dim() == 2 and loc_plan.shape[0] == CAND_PLAN_COLS and (enable is None or enable.numel() == B)
    seg_k = loc_plan.shape[1] // B if B else 1
    assert seg_k >= 1 and loc_plan.shape[1] == B * seg_k
    n_points, dev = int(s["n_points"]), chosen.device
    bitmap = torch.empty(B, max((n_points + 31) // 32, 1), device=dev, dtype=torch.int32)      # zeroed by the entry
    ref_frame = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.check(L.pram_projref_mark(_p(chosen), _p(loc_plan), _p(enable), _p(s["frame_off"]), _p(s["covis_off"]), _p(s["covis_frames"]),
                                   _p(s["point3D_ids"]), _p(s["pt_ids"]), B, seg_k, n_cov, int(s["n_frames"]), int(s["n_covis"]), int(s["n_rows"]),
                                   n_points, _p(bitmap), _p(ref_frame), _st()), "pram_projref_mark")
    return bitmap, ref_frame


def projref_project(bitmap: torch.Tensor, chosen: torch.Tensor, qvec: torch.Tensor, tvec: torch.Tensor, cam_model: torch.Tensor,
                    cam_params: torch.Tensor, image_size: torch.Tensor, store, cap: int):
    """bitmap: projref_mark's; qvec float64 [B * seg_k, 4], tvec [B * seg_k, 3]; cam_model int32 [B], cam_params float64 [B, 8],
    image_size int32 [B, 2] (width, height); ``store``: ReferenceStore.point_tables
    -> (cand_pt int32 [B, cap], cand_uv float64 [B, 2, cap], n_union int32 [B], n_cand int32 [B])."""
    L = _lib.load()
    for t, nm, dt in ((bitmap, "bitmap", torch.int32), (chosen, "chosen", torch.int32), (qvec, "qvec", torch.float64), (tvec, "tvec", torch.float64),
                      (cam_model, "cam_model", torch.int32), (cam_params, "cam_params", torch.float64), (image_size, "image_size", torch.int32)):
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm
    B, cap, s = chosen.shape[0], int(cap), store
    n_points = int(s["n_points"])
    seg_k = qvec.shape[0] // B if B else 1
    assert tuple(chosen.shape) == (B, 3) and seg_k >= 1 and tuple(qvec.shape) == (B * seg_k, 4) and tuple(tvec.shape) == (B * seg_k, 3)
    assert tuple(bitmap.shape) == (B, max((n_points + 31) // 32, 1)) and cam_model.numel() == B and tuple(cam_params.shape) == (B, POSE_CAM_PARAMS)
    assert tuple(image_size.shape) == (B, 2) and s["pt_xyz"].shape[0] >= n_points
    dev = chosen.device
    cand_pt = torch.empty(B, max(cap, 1), device=dev, dtype=torch.int32)
    cand_uv = torch.empty(B, 2, max(cap, 1), device=dev, dtype=torch.float64)
    n_union, n_cand = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    _lib.check(L.pram_projref_project(_p(bitmap), n_points, _p(s["pt_xyz"]), _p(chosen), _p(qvec), _p(tvec), _p(cam_model), _p(cam_params),
                                      _p(image_size), B, seg_k, cap, _p(cand_pt), _p(cand_uv), _p(n_union), _p(n_cand), _st()), "pram_projref_project")
    return cand_pt, cand_uv, n_union, n_cand


def projref_match(q_kpts: torch.Tensor, q_desc: torch.Tensor, counts: torch.Tensor, cand_pt: torch.Tensor, cand_uv: torch.Tensor,
                  n_cand: torch.Tensor, store, threshold: float):
    """q_kpts [B, N, 2], q_desc [B, N, 128], counts int32 [B]; cand_*: projref_project's; ``store``: ReferenceStore.point_tables
    -> (best int32 [B, N] (candidate index, -1 none), d0, d1 float32 [B, N] (+inf: none), accept uint8 [B, N])."""
    L = _lib.load()
    for t, nm, dt in ((q_kpts, "keypoints", torch.float32), (q_desc, "descriptors", torch.float32), (counts, "counts", torch.int32),
                      (cand_pt, "cand_pt", torch.int32), (cand_uv, "cand_uv", torch.float64), (n_cand, "n_cand", torch.int32)):
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm
    B, N, D = q_desc.shape
    cap, s = cand_pt.shape[1], store
    assert D == 128 and tuple(q_kpts.shape) == (B, N, 2) and counts.numel() == B and n_cand.numel() == B
    assert tuple(cand_pt.shape) == (B, cap) and tuple(cand_uv.shape) == (B, 2, cap) and s["pt_desc"].shape[0] >= int(s["n_points"])
    dev = q_desc.device
    best = torch.empty(B, max(N, 1), device=dev, dtype=torch.int32)[:, :N]
    d0, d1 = torch.empty(B, max(N, 1), device=dev)[:, :N], torch.empty(B, max(N, 1), device=dev)[:, :N]
    accept = torch.empty(B, max(N, 1), device=dev, dtype=torch.uint8)[:, :N]
    if N == 0:      # no keypoints: the empty inputs have no storage to hand to the entry
        return best, d0, d1, accept
    _lib.check(L.pram_projref_match(_p(q_kpts), _p(q_desc), _p(counts), B, N, _p(cand_pt), _p(cand_uv), _p(n_cand), cap, _p(s["pt_desc"]),
                                    int(s["n_points"]), float(threshold), _p(best), _p(d0), _p(d1), _p(accept), _st()), "pram_projref_match")
    return best, d0, d1, accept


def projref_correspond(accept: torch.Tensor, best: torch.Tensor, counts: torch.Tensor, q_kpts: torch.Tensor, cand_pt: torch.Tensor,
                       n_cand: torch.Tensor, store, out: Optional[dict] = None) -> dict:
    """-> pram_cand_correspond's layout with N rows per query: matched_keypoint_ids int64 [B, N], matched_keypoints [B, N, 2],
    matched_point3D_ids int64 [B, N], matched_xyzs float64 [B, N, 3], matched_sids int32 [B, N], count int32 [B].  ``out``: buffers
    to write into (the tests pre-fill them)."""
    L = _lib.load()
    for t, nm, dt in ((accept, "accept", torch.uint8), (best, "best", torch.int32), (counts, "counts", torch.int32), (q_kpts, "keypoints", torch.float32),
                      (cand_pt, "cand_pt", torch.int32), (n_cand, "n_cand", torch.int32)):
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm
    B, N = accept.shape
    cap, s = cand_pt.shape[1], store
    assert tuple(best.shape) == (B, N) and tuple(q_kpts.shape) == (B, N, 2) and counts.numel() == B and n_cand.numel() == B and cand_pt.shape[0] == B
    if out is None:
        out = _cor_alloc(B, N, accept.device, MATCH_NOREF_KEYS)
    else:
        assert _cor_chk(out, "out", MATCH_NOREF_KEYS) == (B, max(N, 1))
    if N == 0:      # no keypoints: the empty inputs have no storage to hand to the entry
        out["count"].zero_()
        return out
    _lib.check(L.pram_projref_correspond(_p(accept), _p(best), _p(counts), _p(q_kpts), B, N, _p(cand_pt), _p(n_cand), cap, _p(s["pt_ids"]),
                                         _p(s["pt_xyz"]), _p(s["pt_sid"]), int(s["n_points"]), *[_p(out[k]) for k in MATCH_NOREF_KEYS],
                                         _p(out["count"]), _st()), "pram_projref_correspond")
    return out


# ---- tracking the last frame for a batch of streams (csrc/track.hip; pram_amd/localization/tracker.py drives these) ------------
def _track_state_chk(st: dict):
    """st: the arrays of a TrackState (dict: keypoints, scores, descriptors, counts, xyzs, point3D_ids, seg_ids, ref_frame,
    frame_norm, n_slots, n_max) -> (n_slots, n_max)."""
    S, n_max = int(st["n_slots"]), int(st["n_max"])
    for k, dt, shape in (("keypoints", torch.float32, (S, n_max, 2)), ("scores", torch.float32, (S, n_max)), ("descriptors", torch.float32, (S, n_max, 128)),
                         ("counts", torch.int32, (S,)), ("xyzs", torch.float64, (S, n_max, 3)), ("point3D_ids", _INT64, (S, n_max)),
                         ("seg_ids", torch.int32, (S, n_max)), ("ref_frame", torch.int32, (S,)), ("frame_norm", torch.float32, (S, 3))):
        _chk(st[k], f"state.{k}", dt)
        assert st[k].is_contiguous() and tuple(st[k].shape) == shape, k
    return S, n_max


def track_plan(counts: torch.Tensor, slot: torch.Tensor, st: dict, n: int):
    """counts, slot int32 [B] -> (plan, loc_plan) int32 [CAND_PLAN_COLS, B] (pram_track_plan)."""
    L = _lib.load()
    S, n_max = _track_state_chk(st)
    _chk(counts, "counts", torch.int32)
    _chk(slot, "slot", torch.int32)
    B = counts.numel()
    assert counts.is_contiguous() and slot.is_contiguous() and slot.numel() == B
    plan = torch.empty(CAND_PLAN_COLS, B, device=counts.device, dtype=torch.int32)
    loc_plan = torch.empty(CAND_PLAN_COLS, B, device=counts.device, dtype=torch.int32)
    if B == 0:      # no queries: the empty tensors have no storage to hand to the entry
        return plan, loc_plan
    _lib.check(L.pram_track_plan(_p(counts), _p(slot), _p(st["counts"]), _p(st["ref_frame"]), B, int(n), S, n_max, _p(plan), _p(loc_plan), _st()),
               "pram_track_plan")
    return plan, loc_plan


def track_gather_tables(st: dict, dummy: torch.Tensor) -> dict:
    """The state's arrays under the names cand_gather reads from a ReferenceStore's tables (sel_rows: never read, sel offset -1)."""
    return {"sel_rows": dummy, "descriptors": st["descriptors"], "keypoints": st["keypoints"], "scores": st["scores"], "frame_norm": st["frame_norm"],
            "n_rows": int(st["n_slots"]) * int(st["n_max"])}


def track_correspond(matches0: torch.Tensor, plan: torch.Tensor, st: dict, q_kpts: torch.Tensor, cap: int, out: Optional[dict] = None) -> dict:
    """matches0 int64 [B, >= t0] -> cand_correspond's dict, [B, cap, ...] and count int32 [B] (pram_track_correspond).  ``out``:
    buffers to write into (the tests pre-fill them)."""
    L = _lib.load()
    S, n_max = _track_state_chk(st)
    _chk(matches0, "matches0", _INT64)
    _chk(q_kpts, "keypoints")
    _chk(plan, "plan", torch.int32)
    assert matches0.dim() == 2 and matches0.stride(1) == 1 and q_kpts.is_contiguous() and plan.is_contiguous()
    P, t0 = matches0.shape
    assert tuple(plan.shape) == (CAND_PLAN_COLS, P) and q_kpts.dim() == 3 and q_kpts.shape[0] == P
    n, cap = q_kpts.shape[1], int(cap)
    if out is None:
        out = _cor_alloc(P, cap, matches0.device)
    else:
        _cor_chk(out, "out")
        assert out["matched_sids"].shape[0] == P and out["matched_sids"].shape[1] >= cap
        cap = out["matched_sids"].shape[1]
    _lib.check(L.pram_track_correspond(_p(matches0), matches0.stride(0) if P else t0, _p(plan), _p(q_kpts), n, _p(st["keypoints"]), _p(st["xyzs"]),
                                       _p(st["point3D_ids"]), _p(st["seg_ids"]), S, n_max, P, t0, cap, *[_p(out[k]) for k in MATCH_KEYS],
                                       _p(out["count"]), _st()), "pram_track_correspond")
    return out


def track_filter(cor: dict, mask: torch.Tensor, out: Optional[dict] = None) -> dict:
    """cor: cand_correspond-shaped lists [B, cap, ...] with count; mask uint8 [B, cap] -> the rows r < count[b] with mask != 0, in
    order, in new buffers of the same layout (pram_track_filter)."""
    L = _lib.load()
    B, cap = _cor_chk(cor, "lists")
    _chk(mask, "mask", torch.uint8)
    assert mask.is_contiguous() and tuple(mask.shape) == (B, cap)
    if out is None:
        out = _cor_alloc(B, cap, mask.device)
    else:
        assert _cor_chk(out, "out") == (B, cap)
    _lib.check(L.pram_track_filter(*[_p(cor[k]) for k in MATCH_KEYS], _p(cor["count"]), _p(mask), B, cap, *[_p(out[k]) for k in MATCH_KEYS],
                                   _p(out["count"]), _st()), "pram_track_filter")
    return out


def track_commit(st: dict, q_kpts: torch.Tensor, q_scores: torch.Tensor, q_desc: torch.Tensor, counts: torch.Tensor, seg_ids: Optional[torch.Tensor],
                 slot: torch.Tensor, slot_host, ref_frame: torch.Tensor, q_norm, cor: dict, mask: Optional[torch.Tensor] = None,
                 winner: Optional[torch.Tensor] = None) -> None:
    """In place on the state (pram_track_commit): the queries with slot >= 0 become their slots' last frames and the list rows of
    ``cor`` (with ``mask`` uint8 [B, cap]: those with mask != 0) give their keypoints a point.  slot_host: the slots on the host (a
    sequence of ints), which is what the launcher validates; q_norm = (cx, cy, scale) of the queries' camera."""
    import ctypes
    L = _lib.load()
    S, n_max = _track_state_chk(st)
    for t, nm, dt in ((q_kpts, "keypoints", torch.float32), (q_scores, "scores", torch.float32), (q_desc, "descriptors", torch.float32),
                      (counts, "counts", torch.int32), (slot, "slot", torch.int32), (ref_frame, "ref_frame", torch.int32)) + \
            (((seg_ids, "seg_ids", torch.int32),) if seg_ids is not None else ()) + (((mask, "mask", torch.uint8),) if mask is not None else ()):
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm
    B, n, D = q_desc.shape
    Bc, cap = _cor_chk(cor, "lists", MATCH_POINT_KEYS)
    assert D == 128 and tuple(q_kpts.shape) == (B, n, 2) and tuple(q_scores.shape) == (B, n) and counts.numel() == B and slot.numel() == B
    assert ref_frame.numel() == B and len(slot_host) == B and Bc == B and (seg_ids is None or tuple(seg_ids.shape) == (B, n))
    assert mask is None or tuple(mask.shape) == (B, cap)
    if winner is None:
        winner = torch.empty(B, max(n, 1), device=q_desc.device, dtype=torch.int32)
    _chk(winner, "winner", torch.int32)
    assert winner.is_contiguous() and winner.numel() >= B * n
    host = (ctypes.c_int * max(B, 1))(*[int(s) for s in slot_host])
    _lib.check(L.pram_track_commit(_p(q_kpts), _p(q_scores), _p(q_desc), _p(counts), _p(seg_ids), _p(slot), ctypes.addressof(host), _p(ref_frame), B, n,
                                   float(q_norm[0]), float(q_norm[1]), float(q_norm[2]), *[_p(cor[k]) for k in MATCH_POINT_KEYS], _p(cor["count"]),
                                   _p(mask), cap, _p(st["keypoints"]),
                                   _p(st["scores"]), _p(st["descriptors"]), _p(st["counts"]), _p(st["xyzs"]), _p(st["point3D_ids"]), _p(st["seg_ids"]),
                                   _p(st["ref_frame"]), _p(st["frame_norm"]), S, n_max, _p(winner), _st()), "pram_track_commit")


# ---- the query pre-filter (csrc/prefilter.hip; pram_amd/localization/localizer.py drives it) -------------------------------------
def query_prefilter(keypoints: torch.Tensor, scores: torch.Tensor, descriptors: torch.Tensor, logits: torch.Tensor, seg_ids: torch.Tensor,
                    non_bg_mask: torch.Tensor, n_non_bg: torch.Tensor, counts: torch.Tensor, enable: bool) -> dict:
    """Frame.add_segmentations' filtering of the query for a padded batch (pram_query_prefilter).  keypoints [B, N, 2], scores
    [B, N], descriptors [B, N, D], logits [B, N, C] float32; seg_ids, non_bg_mask [B, N], n_non_bg [B] int32 = seg_epilogue's
    outputs at the filtering threshold; counts [B] int32; enable = the threshold is > 0.  -> dict(keypoints, scores, descriptors,
    logits, seg_ids: new buffers of the same shapes, compacted; counts [B]; kept int32 [B, N]; filtered int32 [B]).  No read-back."""
    L = _lib.load()
    for t, nm, dt in ((keypoints, "keypoints", torch.float32), (scores, "scores", torch.float32), (descriptors, "descriptors", torch.float32),
                      (logits, "logits", torch.float32), (seg_ids, "seg_ids", torch.int32), (non_bg_mask, "non_bg_mask", torch.int32),
                      (n_non_bg, "n_non_bg", torch.int32), (counts, "counts", torch.int32)):
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm
    assert descriptors.dim() == 3 and logits.dim() == 3
    B, N, D = descriptors.shape
    Cc = logits.shape[2]
    assert tuple(keypoints.shape) == (B, N, 2) and tuple(scores.shape) == (B, N) and tuple(logits.shape[:2]) == (B, N)
    assert tuple(seg_ids.shape) == (B, N) and tuple(non_bg_mask.shape) == (B, N) and n_non_bg.numel() == B and counts.numel() == B
    dev = descriptors.device
    out = {"keypoints": torch.empty_like(keypoints), "scores": torch.empty_like(scores), "descriptors": torch.empty_like(descriptors),
           "logits": torch.empty_like(logits), "seg_ids": torch.empty_like(seg_ids), "kept": torch.empty((B, N), device=dev, dtype=torch.int32)}
    if B == 0 or N == 0:      # the empty tensors have no storage to hand to the entry; an empty query keeps nothing, and fires
        out["counts"], out["filtered"] = _filled((B,), dev, torch.int32), _filled((B,), dev, torch.int32, 1 if enable else 0)      # (0 >= 0.4 * 0)
        return out
    out["counts"], out["filtered"] = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    _lib.check(L.pram_query_prefilter(_p(keypoints), _p(scores), _p(descriptors), _p(logits), _p(seg_ids), _p(non_bg_mask), _p(n_non_bg), _p(counts),
                                      1 if enable else 0, B, N, Cc, D, _p(out["keypoints"]), _p(out["scores"]), _p(out["descriptors"]), _p(out["logits"]),
                                      _p(out["seg_ids"]), _p(out["counts"]), _p(out["kept"]), _p(out["filtered"]), _st()), "pram_query_prefilter")
    return out


# ---- map building (csrc/mapbuild.hip; pram_amd/localization/mapbuild.py drives these) ------------------------------------------
MAPBUILD_SHORT_TRACK, MAPBUILD_ROW_LDS, MAPBUILD_MAX_VRF, MAPBUILD_CAM_COLS = 32, 512, 64, 13      # include/pram_hip.h


def _host_offsets(off_host, name: str):
    """A CSR offset table on the host as a ctypes int array (what the entries validate) and its length - 1."""
    import ctypes
    import numpy as np
    a = np.ascontiguousarray(np.asarray(off_host).reshape(-1), dtype=np.int32)
    if a.size < 1:
        raise _lib.PramHipError(f"{name}: an offset table has at least one entry")
    return (ctypes.c_int * a.size).from_buffer_copy(a.tobytes()), a.size - 1


def mapbuild_assign_descriptors(store, trk_off: torch.Tensor, trk_off_host, trk_frame: torch.Tensor, trk_kpt: torch.Tensor,
                                workspace: Optional[torch.Tensor] = None):
    """``store``: the device tables of a ReferenceStore; the tracks as CSR, trk_off int32 [P + 1] with its host copy, trk_frame /
    trk_kpt int32 [E] (store frame index or -1, keypoint index inside the frame) -> (pt_desc float32 [P, 128], pt_choice int32 [P]:
    the position of the chosen entry in the track, -1 for a track with nothing kept).  ``workspace``: uint8, at least
    pram_mapbuild_desc_workspace_bytes; None allocates it."""
    import ctypes
    L = _lib.load()
    for t, nm in ((trk_off, "trk_off"), (trk_frame, "trk_frame"), (trk_kpt, "trk_kpt")):
        _chk(t, nm, torch.int32)
        assert t.is_contiguous(), nm
    s = store
    _chk(s["descriptors"], "descriptors")
    host, P = _host_offsets(trk_off_host, "trk_off")
    E = int(host[P])
    assert trk_off.numel() >= P + 1 and trk_frame.numel() >= E and trk_kpt.numel() >= E and s["descriptors"].is_contiguous() and s["descriptors"].shape[-1] == 128
    dev = trk_off.device
    need = int(L.pram_mapbuild_desc_workspace_bytes(ctypes.addressof(host), P))
    if workspace is None:
        workspace = torch.empty(max(need, 8), device=dev, dtype=torch.uint8)
    _chk(workspace, "workspace", torch.uint8)
    pt_desc = torch.empty(max(P, 1), 128, device=dev, dtype=torch.float32)
    pt_choice = torch.empty(max(P, 1), device=dev, dtype=torch.int32)
    _lib.check(L.pram_mapbuild_assign_descriptors(_p(s["descriptors"]), _p(s["frame_off"]), int(s["n_frames"]), int(s["n_rows"]), _p(trk_off),
                                                  ctypes.addressof(host), _p(trk_frame), _p(trk_kpt), P, _p(workspace), workspace.numel(),
                                                  _p(pt_desc), _p(pt_choice), _st()), "pram_mapbuild_assign_descriptors")
    return pt_desc[:P], pt_choice[:P]


def mapbuild_select_frames(store, pt_xyz: torch.Tensor, lm_off: torch.Tensor, lm_off_host, lm_points: torch.Tensor, frame_ignored: torch.Tensor,
                           frame_cams: torch.Tensor, min_obs: int = 120, topk_imgs: int = 500, n_vrf: int = 10, min_cover_ratio: float = 0.9,
                           gain_floor: float = 0.01, workspace: Optional[torch.Tensor] = None):
    """``store``: the device tables of a ReferenceStore (rows and point table); pt_xyz float64 [n_points, 3] aligned with pt_ids; the
    landmarks as CSR, lm_off int32 [L + 1] with its host copy and lm_points int64 [sum]; frame_ignored int32 [F]; frame_cams float64
    [F, MAPBUILD_CAM_COLS] (qvec, tvec, fx, fy, cx, cy, width, height) -> (lm_vrf int32 [L, n_vrf] store frame indices padded with
    -1, lm_vrf_n int32 [L]).  ``workspace``: uint8, at least pram_mapbuild_vrf_workspace_bytes; None allocates it."""
    import ctypes
    L = _lib.load()
    s = store
    for t, nm, dt in ((pt_xyz, "pt_xyz", torch.float64), (lm_off, "lm_off", torch.int32), (lm_points, "lm_points", _INT64),
                      (frame_ignored, "frame_ignored", torch.int32), (frame_cams, "frame_cams", torch.float64)):
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm
    host, n_lm = _host_offsets(lm_off_host, "lm_off")
    total = int(host[n_lm])
    F, n_points, n_vrf = int(s["n_frames"]), int(s["n_points"]), int(n_vrf)
    assert lm_off.numel() >= n_lm + 1 and lm_points.numel() >= total and frame_ignored.numel() >= F and frame_cams.numel() >= F * MAPBUILD_CAM_COLS
    assert pt_xyz.numel() >= 3 * n_points
    dev = lm_off.device
    need = int(L.pram_mapbuild_vrf_workspace_bytes(n_lm, max(total, 0), F))
    if workspace is None:
        workspace = torch.empty(max(need, 8), device=dev, dtype=torch.uint8)
    _chk(workspace, "workspace", torch.uint8)
    lm_vrf = torch.empty(max(n_lm, 1), max(n_vrf, 1), device=dev, dtype=torch.int32)
    lm_vrf_n = torch.empty(max(n_lm, 1), device=dev, dtype=torch.int32)
    _lib.check(L.pram_mapbuild_select_frames(_p(s["point3D_ids"]), _p(s["frame_off"]), F, int(s["n_rows"]), _p(s["pt_ids"]), _p(s["pt_off"]),
                                             _p(s["pt_frames"]), n_points, int(s["n_pt_entries"]), _p(pt_xyz), _p(lm_off), ctypes.addressof(host),
                                             _p(lm_points), n_lm, _p(frame_ignored), _p(frame_cams), int(min_obs), int(topk_imgs), n_vrf,
                                             float(min_cover_ratio), float(gain_floor), _p(workspace), workspace.numel(), _p(lm_vrf), _p(lm_vrf_n),
                                             _st()), "pram_mapbuild_select_frames")
    return lm_vrf[:n_lm], lm_vrf_n[:n_lm]


# ---- map compression (csrc/compress.hip; pram_amd/localization/compress.py drives these) --------------------------------------
COMPRESS_ROW_TILE, COMPRESS_KPT_TILE = 256, 256      # include/pram_hip.h


def _host_ints(a, name: str):
    """A host table as a ctypes int array (never empty behind its pointer) and its length."""
    import ctypes
    import numpy as np
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32)
    return (ctypes.c_int * max(a.size, 1)).from_buffer_copy(a.tobytes() if a.size else b"\0\0\0\0"), a.size


def compress_workspace(store, device) -> torch.Tensor:
    need = int(_lib.load().pram_compress_workspace_bytes(int(store["n_rows"]), int(store["covisibility_frame"])))
    return torch.empty(max(need, 8), device=device, dtype=torch.uint8)


def compress_select(store, frame_off_host, covis_off_host, covis_frames_host, vrf_host, pt_xyz: torch.Tensor, xys: torch.Tensor,
                    frame_cams: torch.Tensor, radius: float, workspace: Optional[torch.Tensor] = None):
    """``store``: the device tables of a ReferenceStore (rows and point ids); the host copies of frame_off and of the covisibility
    graph, and the reference frames in order, as int arrays; pt_xyz float64 [n_points, 3]; xys float64 [n_rows, 2]; frame_cams
    float64 [F, MAPBUILD_CAM_COLS] -> (ret_order int32 [F]: place in the retained order or -1, list_cnt int32 [F], list_pt int32
    [n_rows]: frame f's kept rows as point table indices at frame_off[f] ..).  Nothing is read back."""
    import ctypes
    L = _lib.load()
    s = store
    for t, nm in ((pt_xyz, "pt_xyz"), (xys, "xys"), (frame_cams, "frame_cams")):
        _chk(t, nm, torch.float64)
        assert t.is_contiguous(), nm
    F, n_rows, n_points, cov = int(s["n_frames"]), int(s["n_rows"]), int(s["n_points"]), int(s["covisibility_frame"])
    fo, n_fo = _host_ints(frame_off_host, "frame_off")
    co, n_co = _host_ints(covis_off_host, "covis_off")
    cf, n_cf = _host_ints(covis_frames_host, "covis_frames")
    vh, n_vrf = _host_ints(vrf_host, "vrf")
    if n_fo != F + 1 or n_co != F + 1 or n_cf < int(co[F]) or F < 1:
        raise _lib.PramHipError(f"compress_select: frame_off and covis_off need {F + 1} entries (at least one frame), covis_frames {int(co[F]) if n_co == F + 1 else '?'}")
    assert pt_xyz.numel() >= 3 * n_points and xys.numel() >= 2 * n_rows and frame_cams.numel() >= F * MAPBUILD_CAM_COLS
    dev = pt_xyz.device
    if workspace is None:
        workspace = compress_workspace(s, dev)
    _chk(workspace, "workspace", torch.uint8)
    ret_order = torch.empty(F, device=dev, dtype=torch.int32)
    list_cnt = torch.empty(F, device=dev, dtype=torch.int32)
    list_pt = torch.empty(max(n_rows, 1), device=dev, dtype=torch.int32)
    _lib.check(L.pram_compress_select(_p(s["point3D_ids"]), _p(s["frame_off"]), ctypes.addressof(fo), F, n_rows, _p(s["pt_ids"]), n_points, _p(pt_xyz),
                                      _p(xys), _p(frame_cams), ctypes.addressof(co), ctypes.addressof(cf), cov, ctypes.addressof(vh), n_vrf,
                                      float(radius), _p(workspace), workspace.numel(), _p(ret_order), _p(list_cnt), _p(list_pt), _st()),
               "pram_compress_select")
    return ret_order, list_cnt, list_pt


def compress_sparsify(store, frame_cams: torch.Tensor, pt_xyz: torch.Tensor, pt_score: torch.Tensor, radius: float, nkpts: int,
                      list_pt: torch.Tensor, list_cnt: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> None:
    """In place on (list_pt, list_cnt) of :func:`compress_select`: every frame listing more than ``nkpts`` points keeps the best
    point (pt_score int32 [n_points], the earlier on a tie) of every cell of ``radius`` pixels, in the order the cells appear."""
    L = _lib.load()
    s = store
    for t, nm, dt in ((frame_cams, "frame_cams", torch.float64), (pt_xyz, "pt_xyz", torch.float64), (pt_score, "pt_score", torch.int32),
                      (list_pt, "list_pt", torch.int32), (list_cnt, "list_cnt", torch.int32)):
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm
    F, n_rows, n_points = int(s["n_frames"]), int(s["n_rows"]), int(s["n_points"])
    assert pt_xyz.numel() >= 3 * n_points and pt_score.numel() >= n_points and frame_cams.numel() >= F * MAPBUILD_CAM_COLS
    assert list_pt.numel() >= n_rows and list_cnt.numel() >= F
    if workspace is None:
        workspace = compress_workspace(s, pt_xyz.device)
    _chk(workspace, "workspace", torch.uint8)
    _lib.check(L.pram_compress_sparsify(_p(s["frame_off"]), F, n_rows, _p(frame_cams), _p(pt_xyz), _p(pt_score), n_points, float(radius), int(nkpts),
                                        _p(workspace), workspace.numel(), _p(list_pt), _p(list_cnt), _st()), "pram_compress_sparsify")


def compress_rows(row_frame: torch.Tensor, row_point: torch.Tensor, n_frames: int, frame_cams: torch.Tensor, pt_ids: torch.Tensor,
                  pt_xyz: torch.Tensor, pt_desc: torch.Tensor, pt_sid: torch.Tensor, pt_err: torch.Tensor, n_points: int) -> dict:
    """Row i of a compressed map: point row_point[i] (index into the point table) seen from frame row_frame[i] -> dict(keypoints
    float64 [n, 3] (u, v, score), xyzs float64 [n, 3], descriptors float32 [n, 128], keypoint_segs int32 [n], point3D_ids int64 [n])."""
    L = _lib.load()
    for t, nm, dt in ((row_frame, "row_frame", torch.int32), (row_point, "row_point", torch.int32), (frame_cams, "frame_cams", torch.float64),
                      (pt_ids, "pt_ids", _INT64), (pt_xyz, "pt_xyz", torch.float64), (pt_desc, "pt_desc", torch.float32),
                      (pt_sid, "pt_sid", torch.int32), (pt_err, "pt_err", torch.float64)):
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm
    n = int(row_frame.numel())
    assert row_point.numel() == n and frame_cams.numel() >= int(n_frames) * MAPBUILD_CAM_COLS and pt_ids.numel() >= n_points
    assert pt_xyz.numel() >= 3 * n_points and pt_desc.numel() >= 128 * n_points and pt_sid.numel() >= n_points and pt_err.numel() >= n_points
    dev = row_frame.device
    m = max(n, 1)
    out = {"keypoints": torch.empty(m, 3, device=dev, dtype=torch.float64), "xyzs": torch.empty(m, 3, device=dev, dtype=torch.float64),
           "descriptors": torch.empty(m, 128, device=dev, dtype=torch.float32), "keypoint_segs": torch.empty(m, device=dev, dtype=torch.int32),
           "point3D_ids": torch.empty(m, device=dev, dtype=_INT64)}
    _lib.check(L.pram_compress_rows(_p(row_frame), _p(row_point), n, int(n_frames), int(n_points), _p(frame_cams), _p(pt_ids), _p(pt_xyz), _p(pt_desc),
                                    _p(pt_sid), _p(pt_err), _p(out["keypoints"]), _p(out["xyzs"]), _p(out["descriptors"]), _p(out["keypoint_segs"]),
                                    _p(out["point3D_ids"]), _st()), "pram_compress_rows")
    return {k: v[:n] for k, v in out.items()}


# ---- k-means labelling (csrc/kmeans.hip; pram_amd/localization/labelling.py drives these) --------------------------------------
KMEANS_BLOCK, KMEANS_MAX_K, KMEANS_MAX_TRIALS, KMEANS_STATE_WORDS = 1024, 4096, 10, 8      # include/pram_hip.h
KMEANS_DONE, KMEANS_ITER, KMEANS_STRICT, KMEANS_RELOC = 0, 1, 2, 3      # words of the state


def _kmeans_x(x: torch.Tensor, name: str = "x") -> int:
    _chk(x, name, torch.float64)
    if x.dim() != 2 or x.shape[1] != 3 or not x.is_contiguous():
        raise _lib.PramHipError(f"{name}: expected a contiguous float64 [n, 3] tensor, got {tuple(x.shape)}")
    return int(x.shape[0])


def kmeans_workspace(n: int, k: int, device) -> torch.Tensor:
    need = int(_lib.load().pram_kmeans_workspace_bytes(int(n), int(k)))
    if need == 0:
        raise _lib.PramHipError(f"kmeans: needs 1 <= n < 2^31 and 1 <= k <= min(n, {KMEANS_MAX_K}), got n = {n}, k = {k}")
    return torch.empty(need, device=device, dtype=torch.uint8)


def kmeans_init_pp(x: torch.Tensor, k: int, first: int, rand: torch.Tensor, workspace: Optional[torch.Tensor] = None):
    """sklearn's k-means++ on the centred points x float64 [n, 3] with the host's random numbers: ``first`` the first seed, rand
    float64 [k - 1, T] the uniform numbers of every step -> (seeds int32 [k]: the chosen points, centers float64 [k, 3])."""
    L = _lib.load()
    n, k = _kmeans_x(x), int(k)
    _chk(rand, "rand", torch.float64)
    T = int(rand.shape[1]) if rand.dim() == 2 else 0
    if rand.dim() != 2 or not rand.is_contiguous() or rand.shape[0] < k - 1 or T < 1:
        raise _lib.PramHipError(f"rand: expected a contiguous float64 [k - 1, T] tensor with T >= 1, got {tuple(rand.shape)}")
    if workspace is None:
        workspace = kmeans_workspace(n, k, x.device)
    _chk(workspace, "workspace", torch.uint8)
    seeds = torch.empty(max(k, 1), device=x.device, dtype=torch.int32)
    centers = torch.empty(max(k, 1), 3, device=x.device, dtype=torch.float64)
    _lib.check(L.pram_kmeans_init_pp(_p(x), n, k, int(first), _p(rand), T, _p(workspace), workspace.numel(), _p(seeds), _p(centers), _st()),
               "pram_kmeans_init_pp")
    return seeds, centers


def kmeans_buffers(n: int, device) -> dict:
    """The outputs and the state of :func:`kmeans_lloyd`, which carries them from one group of iterations to the next."""
    return {"labels": torch.empty(n, device=device, dtype=torch.int32), "dist": torch.empty(n, device=device, dtype=torch.float64),
            "state": torch.zeros(KMEANS_STATE_WORDS, device=device, dtype=torch.int32), "inertia": torch.zeros(2, device=device, dtype=torch.float64)}


def kmeans_lloyd(x: torch.Tensor, centers: torch.Tensor, tol_abs: float, max_iter: int, first_iter: int, n_iters: int, finish: bool,
                 buffers: dict, workspace: torch.Tensor) -> None:
    """Enqueues Lloyd iterations first_iter .. first_iter + n_iters - 1 on ``centers`` float64 [k, 3] (in place) and, with
    ``finish``, the final labels, distances and inertia into ``buffers`` (:func:`kmeans_buffers`).  buffers["state"] says when the
    iterations are done (word KMEANS_DONE); later iterations then return at once.  Nothing is read back here."""
    L = _lib.load()
    n = _kmeans_x(x)
    k = _kmeans_x(centers, "centers")
    _chk(workspace, "workspace", torch.uint8)
    for nm, dt, cnt in (("labels", torch.int32, n), ("dist", torch.float64, n), ("state", torch.int32, KMEANS_STATE_WORDS), ("inertia", torch.float64, 2)):
        _chk(buffers[nm], nm, dt)
        assert buffers[nm].is_contiguous() and buffers[nm].numel() >= cnt, nm
    _lib.check(L.pram_kmeans_lloyd(_p(x), n, k, _p(centers), float(tol_abs), int(max_iter), int(first_iter), int(n_iters), int(bool(finish)),
                                   _p(workspace), workspace.numel(), _p(buffers["labels"]), _p(buffers["dist"]), _p(buffers["state"]),
                                   _p(buffers["inertia"]), _st()), "pram_kmeans_lloyd")


def kmeans_assign(x: torch.Tensor, centers: torch.Tensor):
    """One assignment step: x float64 [n, 3], centers float64 [k, 3] (k <= n) -> (labels int32 [n], squared distance float64 [n]);
    the lowest centre index wins a tie."""
    L = _lib.load()
    n = _kmeans_x(x)
    k = _kmeans_x(centers, "centers")
    labels = torch.empty(max(n, 1), device=x.device, dtype=torch.int32)
    dist = torch.empty(max(n, 1), device=x.device, dtype=torch.float64)
    _lib.check(L.pram_kmeans_assign(_p(x), n, _p(centers), k, _p(labels), _p(dist), _st()), "pram_kmeans_assign")
    return labels[:n], dist[:n]


# ---- triangulation (csrc/triangulate.hip; pram_amd/localization/triangulation.py drives these) --------------------------------
TRI_GN_STEPS, TRI_FRAME_COLS, TRI_CC_STATE_WORDS = 5, 16, 4      # include/pram_hip.h
TRI_CC_DONE = 1      # the word of the components' state that says the labels are final
TRI_ROW_FREE, TRI_ROW_TAKEN, TRI_ROW_DEAD = 0, 1, 2      # include/pram_hip.h


def _tri_chk(items):
    for t, nm, dt in items:
        _chk(t, nm, dt)
        assert t.is_contiguous(), nm


def _tri_views(norm, keypoints, table, cam_model, cam_params, n_frames: int, n_rows: int):
    """The five tensors stage 2b and stage 4 read of the frame table, and their sizes."""
    _tri_chk(((norm, "norm", torch.float64), (keypoints, "keypoints", torch.float32), (table, "table", torch.float64),
              (cam_model, "cam_model", torch.int32), (cam_params, "cam_params", torch.float64)))
    assert norm.numel() >= 2 * n_rows and keypoints.numel() >= 2 * n_rows and table.numel() >= TRI_FRAME_COLS * n_frames
    assert cam_model.numel() >= n_frames and cam_params.numel() >= POSE_CAM_PARAMS * n_frames


def _tri_workspace(need: int, refusal: str, workspace: Optional[torch.Tensor], device) -> torch.Tensor:
    """need: what the entry's *_workspace_bytes returned (0: it refuses the sizes) -> ``workspace`` checked, or a new one."""
    if need == 0:
        raise _lib.PramHipError(refusal)
    if workspace is None:
        workspace = torch.empty(need, device=device, dtype=torch.uint8)
    _chk(workspace, "workspace", torch.uint8)
    return workspace


def _tri_models(cam_model_host, n_frames: int):
    import ctypes
    assert len(cam_model_host) == n_frames
    return (ctypes.c_int * max(n_frames, 1))(*[int(m) for m in cam_model_host])


def tri_frames(qvec: torch.Tensor, tvec: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor, cam_model_host) -> torch.Tensor:
    """cam_from_world poses qvec float64 [F, 4] (w, x, y, z), tvec float64 [F, 3] and the frames' cameras (cam_model int32 [F],
    cam_params float64 [F, POSE_CAM_PARAMS], cam_model_host: the ids on the host) -> the frame table float64 [F, TRI_FRAME_COLS]
    that tri_verify and tri_triangulate read.  Every tensor holds one row at least (the rows beyond F are not read)."""
    import ctypes
    L = _lib.load()
    _tri_chk(((qvec, "qvec", torch.float64), (tvec, "tvec", torch.float64), (cam_model, "cam_model", torch.int32),
              (cam_params, "cam_params", torch.float64)))
    F = len(cam_model_host)
    assert qvec.numel() >= 4 * F and tvec.numel() >= 3 * F and cam_model.numel() >= F and cam_params.numel() >= POSE_CAM_PARAMS * F
    host = _tri_models(cam_model_host, F)
    table = torch.empty(max(F, 1), TRI_FRAME_COLS, device=qvec.device, dtype=torch.float64)
    _lib.check(L.pram_tri_frames(_p(qvec), _p(tvec), _p(cam_model), _p(cam_params), ctypes.addressof(host), F, _p(table), _st()), "pram_tri_frames")
    return table


def tri_normalize(keypoints: torch.Tensor, frame_off: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor, cam_model_host,
                  n_rows: int, pixel_offset: float) -> torch.Tensor:
    """keypoints float32 [n_rows, 2] of all frames, frame_off int32 [F + 1] -> float64 [n_rows, 2] on the normalised plane of each
    row's frame, (x + pixel_offset, y + pixel_offset) undistorted as pose_prepare does."""
    import ctypes
    L = _lib.load()
    _tri_chk(((keypoints, "keypoints", torch.float32), (frame_off, "frame_off", torch.int32), (cam_model, "cam_model", torch.int32),
              (cam_params, "cam_params", torch.float64)))
    F, n_rows = len(cam_model_host), int(n_rows)
    assert keypoints.numel() >= 2 * n_rows and frame_off.numel() >= F + 1 and cam_model.numel() >= F and cam_params.numel() >= POSE_CAM_PARAMS * F
    host = _tri_models(cam_model_host, F)
    norm = torch.empty(max(n_rows, 1), 2, device=keypoints.device, dtype=torch.float64)
    _lib.check(L.pram_tri_normalize(_p(keypoints), _p(frame_off), _p(cam_model), _p(cam_params), ctypes.addressof(host), F, n_rows,
                                    float(pixel_offset), _p(norm), _st()), "pram_tri_normalize")
    return norm


def tri_verify(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, matches: torch.Tensor,
               table: torch.Tensor, n_frames: int, n_pairs: int, n_matches: int, max_error: float) -> dict:
    """norm: tri_normalize with offset 0; pairs int32 [Pn, 2] frame indices; the matches as CSR, match_off int32 [Pn + 1] and
    matches int32 [M, 2] -> keep uint8 [M], kept int32 [M, 2] (pair p's kept matches from match_off[p] on, original order), edges
    int32 [M, 2] (rows, -1 where dropped), count int32 [Pn]."""
    L = _lib.load()
    _tri_chk(((norm, "norm", torch.float64), (frame_off, "frame_off", torch.int32), (pairs, "pairs", torch.int32),
              (match_off, "match_off", torch.int32), (matches, "matches", torch.int32), (table, "table", torch.float64)))
    F, Pn, M = int(n_frames), int(n_pairs), int(n_matches)
    assert frame_off.numel() >= F + 1 and pairs.numel() >= 2 * Pn and match_off.numel() >= Pn + 1 and matches.numel() >= 2 * M
    assert table.numel() >= TRI_FRAME_COLS * F
    dev = norm.device
    out = {"keep": torch.empty(max(M, 1), device=dev, dtype=torch.uint8), "kept": torch.empty(max(M, 1), 2, device=dev, dtype=torch.int32),
           "edges": torch.empty(max(M, 1), 2, device=dev, dtype=torch.int32), "count": torch.empty(max(Pn, 1), device=dev, dtype=torch.int32)}
    _lib.check(L.pram_tri_verify(_p(norm), _p(frame_off), _p(pairs), _p(match_off), _p(matches), _p(table), F, Pn, M, float(max_error),
                                 _p(out["keep"]), _p(out["kept"]), _p(out["edges"]), _p(out["count"]), _st()), "pram_tri_verify")
    return out


def tri_components(edges: torch.Tensor, n_edges: int, n_rows: int, first_round: int, n_rounds: int, label: torch.Tensor, state: torch.Tensor):
    """Rounds first_round .. first_round + n_rounds - 1 of the connected components over rows (edges int32 [n_edges, 2]) on label
    int32 [n_rows] and state int32 [TRI_CC_STATE_WORDS]; state[TRI_CC_DONE] says when label holds every row's smallest row."""
    L = _lib.load()
    _tri_chk(((edges, "edges", torch.int32), (label, "label", torch.int32), (state, "state", torch.int32)))
    assert edges.numel() >= 2 * int(n_edges) and label.numel() >= int(n_rows) and state.numel() >= TRI_CC_STATE_WORDS
    _lib.check(L.pram_tri_components(_p(edges), int(n_edges), int(n_rows), int(first_round), int(n_rounds), _p(label), _p(state), _st()),
               "pram_tri_components")


def tri_tracks(label: torch.Tensor, frame_off: torch.Tensor, n_frames: int, n_rows: int, workspace: Optional[torch.Tensor] = None) -> dict:
    """label int32 [n_rows] (tri_components) -> the tracks as CSR, sized for the worst case: trk_off int32 [n_rows // 2 + 2],
    trk_label int32 [n_rows // 2 + 1], trk_row / trk_frame / trk_kpt int32 [n_rows], and sizes int32 [2] = (tracks, entries), all on
    the device.  ``workspace``: uint8, at least pram_tri_tracks_workspace_bytes; None allocates it."""
    L = _lib.load()
    _tri_chk(((label, "label", torch.int32), (frame_off, "frame_off", torch.int32)))
    F, n = int(n_frames), int(n_rows)
    assert label.numel() >= n and frame_off.numel() >= F + 1
    dev = label.device
    workspace = _tri_workspace(int(L.pram_tri_tracks_workspace_bytes(n)), "pram_tri_tracks: more than 2^30 rows", workspace, dev)
    i32 = lambda m: torch.empty(max(m, 1), device=dev, dtype=torch.int32)
    out = {"trk_off": i32(n // 2 + 2), "trk_label": i32(n // 2 + 1), "trk_row": i32(n), "trk_frame": i32(n), "trk_kpt": i32(n), "sizes": i32(2)}
    _lib.check(L.pram_tri_tracks(_p(label), _p(frame_off), F, n, _p(workspace), workspace.numel(), _p(out["trk_off"]), _p(out["trk_label"]),
                                 _p(out["trk_row"]), _p(out["trk_frame"]), _p(out["trk_kpt"]), _p(out["sizes"]), _st()), "pram_tri_tracks")
    return out


def tri_triangulate(norm: torch.Tensor, keypoints: torch.Tensor, table: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor,
                    trk_off: torch.Tensor, trk_label: torch.Tensor, trk_row: torch.Tensor, trk_frame: torch.Tensor, n_tracks: int,
                    n_entries: int, n_frames: int, n_rows: int, trials: int = 128, seed: int = 0, min_tri_angle: float = 0.026179938779914945,
                    max_reproj_error: float = 4.0) -> dict:
    """norm: tri_normalize with offset 0.5; the tracks of tri_tracks (or a caller's own table) -> accept int32 [T], xyz float64
    [T, 3], error float64 [T], kept int32 [T], best int32 [T] (the winning hypothesis, -1: none), entry_keep uint8 [E], entry_error
    float64 [E].  min_tri_angle in radians."""
    L = _lib.load()
    T, E, F, n = int(n_tracks), int(n_entries), int(n_frames), int(n_rows)
    _tri_views(norm, keypoints, table, cam_model, cam_params, F, n)
    _tri_chk(((trk_off, "trk_off", torch.int32), (trk_label, "trk_label", torch.int32), (trk_row, "trk_row", torch.int32),
              (trk_frame, "trk_frame", torch.int32)))
    assert trk_off.numel() >= T + 1 and trk_label.numel() >= T and trk_row.numel() >= E and trk_frame.numel() >= E
    dev = norm.device
    new = lambda m, dt, *rest: torch.empty(max(m, 1), *rest, device=dev, dtype=dt)
    out = {"accept": new(T, torch.int32), "xyz": new(T, torch.float64, 3), "error": new(T, torch.float64), "kept": new(T, torch.int32),
           "best": new(T, torch.int32), "entry_keep": new(E, torch.uint8), "entry_error": new(E, torch.float64)}
    _lib.check(L.pram_tri_triangulate(_p(norm), _p(keypoints), _p(table), _p(cam_model), _p(cam_params), _p(trk_off), _p(trk_label), _p(trk_row),
                                      _p(trk_frame), T, E, F, n, int(trials), int(seed) & 0xFFFFFFFFFFFFFFFF, float(min_tri_angle),
                                      float(max_reproj_error), _p(out["accept"]), _p(out["xyz"]), _p(out["error"]), _p(out["kept"]), _p(out["best"]),
                                      _p(out["entry_keep"]), _p(out["entry_error"]), _st()), "pram_tri_triangulate")
    return out


def tri_adjacency(edges: torch.Tensor, n_edges: int, frame_off: torch.Tensor, n_frames: int, n_rows: int,
                  workspace: Optional[torch.Tensor] = None) -> dict:
    """edges int32 [n_edges, 2] rows (an edge with an end outside [0, n_rows) or with equal ends is skipped) -> the rows' adjacency
    on the device: adj_off int32 [n_rows + 1], adj int32 [2 * n_edges] (adj_off[n_rows] of them written, every row's list
    ascending, duplicates kept) and row_frame int32 [n_rows].  ``workspace``: uint8, at least
    pram_tri_adjacency_workspace_bytes; None allocates it."""
    L = _lib.load()
    _tri_chk(((edges, "edges", torch.int32), (frame_off, "frame_off", torch.int32)))
    m, F, n = int(n_edges), int(n_frames), int(n_rows)
    assert edges.numel() >= 2 * m and frame_off.numel() >= F + 1
    dev = edges.device
    workspace = _tri_workspace(int(L.pram_tri_adjacency_workspace_bytes(n, m)), "pram_tri_adjacency: more than 2^30 rows or 2^30 - 1 edges",
                               workspace, dev)
    i32 = lambda k: torch.empty(max(k, 1), device=dev, dtype=torch.int32)
    out = {"adj_off": i32(n + 1), "adj": i32(2 * m), "row_frame": i32(n)}
    _lib.check(L.pram_tri_adjacency(_p(edges), m, _p(frame_off), F, n, _p(workspace), workspace.numel(), _p(out["adj_off"]), _p(out["adj"]),
                                    _p(out["row_frame"]), _st()), "pram_tri_adjacency")
    return out


def tri_support(norm: torch.Tensor, keypoints: torch.Tensor, table: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor,
                edges: torch.Tensor, n_edges: int, adj_off: torch.Tensor, adj: torch.Tensor, row_frame: torch.Tensor, n_frames: int,
                n_rows: int, min_tri_angle: float = 0.026179938779914945, max_reproj_error: float = 4.0, min_support: int = 1) -> dict:
    """norm: tri_normalize with offset 0.5; adj_off / adj / row_frame: tri_adjacency over the same edges -> support int32 [n_edges]
    (the witnesses of third frames that confirm the edge) and edges int32 [n_edges, 2]: the edge where support >= min_support,
    (-1, -1) elsewhere.  min_tri_angle in radians."""
    L = _lib.load()
    m, F, n = int(n_edges), int(n_frames), int(n_rows)
    _tri_views(norm, keypoints, table, cam_model, cam_params, F, n)
    _tri_chk(((edges, "edges", torch.int32), (adj_off, "adj_off", torch.int32), (adj, "adj", torch.int32), (row_frame, "row_frame", torch.int32)))
    assert edges.numel() >= 2 * m and adj_off.numel() >= n + 1 and adj.numel() >= 2 * m and row_frame.numel() >= n
    dev = norm.device
    out = {"support": torch.empty(max(m, 1), device=dev, dtype=torch.int32), "edges": torch.empty(max(m, 1), 2, device=dev, dtype=torch.int32)}
    _lib.check(L.pram_tri_support(_p(norm), _p(keypoints), _p(table), _p(cam_model), _p(cam_params), _p(edges), m, _p(adj_off), _p(adj),
                                  _p(row_frame), F, n, float(min_tri_angle), float(max_reproj_error), int(min_support), _p(out["support"]),
                                  _p(out["edges"]), _st()), "pram_tri_support")
    return out


def tri_split(trk_off: torch.Tensor, trk_row: torch.Tensor, n_tracks: int, n_entries: int, accept: torch.Tensor, entry_keep: torch.Tensor,
              edges: torch.Tensor, n_edges: int, n_rows: int, state: Optional[torch.Tensor] = None) -> dict:
    """One round's track table (tri_tracks) and results (tri_triangulate's accept and entry_keep) and the edges the first round's
    tracks came from -> state uint8 [n_rows] (TRI_ROW_*; ``state`` updated in place, None: a new one that starts all DEAD), edges
    int32 [n_edges, 2]: the edge where both ends are FREE, (-1, -1) elsewhere, and n_live int32 [1], the number of such edges, on
    the device."""
    L = _lib.load()
    _tri_chk(((trk_off, "trk_off", torch.int32), (trk_row, "trk_row", torch.int32), (accept, "accept", torch.int32),
              (entry_keep, "entry_keep", torch.uint8), (edges, "edges", torch.int32)))
    T, E, m, n = int(n_tracks), int(n_entries), int(n_edges), int(n_rows)
    assert trk_off.numel() >= T + 1 and trk_row.numel() >= E and accept.numel() >= T and entry_keep.numel() >= E and edges.numel() >= 2 * m
    dev = edges.device
    first = state is None
    if first:
        state = torch.empty(max(n, 1), device=dev, dtype=torch.uint8)
    _tri_chk(((state, "state", torch.uint8),))
    assert state.numel() >= n
    out = {"state": state, "edges": torch.empty(max(m, 1), 2, device=dev, dtype=torch.int32), "n_live": torch.empty(1, device=dev, dtype=torch.int32)}
    _lib.check(L.pram_tri_split(_p(trk_off), _p(trk_row), T, E, _p(accept), _p(entry_keep), _p(edges), m, n, int(first), _p(state),
                                _p(out["edges"]), _p(out["n_live"]), _st()), "pram_tri_split")
    return out


# ---- two-view geometry without poses (csrc/twoview.hip; pram_amd/localization/twoview.py drives these) ------------------------
TWOVIEW_MAX_SOL = 10      # PRAM_TWOVIEW_MAX_SOL
TWOVIEW_TRIAL_BYTES = TWOVIEW_MAX_SOL * (9 * 8 + 4 + 8) + 4      # hypotheses, counts, residual sums and n_sol of one trial


def _twoview_views(norm, frame_off, pairs, match_off, matches, n_frames: int, n_pairs: int, n_matches: int):
    """The five tensors every two-view entry reads of the frame table and the match CSR, and their sizes."""
    _tri_chk(((norm, "norm", torch.float64), (frame_off, "frame_off", torch.int32), (pairs, "pairs", torch.int32),
              (match_off, "match_off", torch.int32), (matches, "matches", torch.int32)))
    assert frame_off.numel() >= n_frames + 1 and pairs.numel() >= 2 * n_pairs and match_off.numel() >= n_pairs + 1 and matches.numel() >= 2 * n_matches


def _twoview_cams(cam_model, cam_params, n_frames: int):
    _tri_chk(((cam_model, "cam_model", torch.int32), (cam_params, "cam_params", torch.float64)))
    assert cam_model.numel() >= n_frames and cam_params.numel() >= POSE_CAM_PARAMS * n_frames


def twoview_hypotheses(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, matches: torch.Tensor,
                       n_frames: int, n_pairs: int, n_matches: int, first_pair: int = 0, trials: int = 1024, seed: int = 0,
                       return_fives: bool = False) -> dict:
    """norm: tri_normalize with offset 0.5; pairs int32 [Pn, 2]; the matches as CSR (match_off int32 [Pn + 1], matches int32 [M, 2])
    -> E float64 [Pn, trials, TWOVIEW_MAX_SOL, 9] (the kept roots of every five-point sample first, zeros behind), n_sol int32
    [Pn, trials] and, with return_fives, fives int32 [Pn, trials, 5].  first_pair: the position of pairs[0] among all processed
    pairs (the sampler's key)."""
    L = _lib.load()
    F, Pn, M, T = int(n_frames), int(n_pairs), int(n_matches), int(trials)
    _twoview_views(norm, frame_off, pairs, match_off, matches, F, Pn, M)
    dev = norm.device
    out = {"E": torch.empty(max(Pn, 1), T, TWOVIEW_MAX_SOL, 9, device=dev, dtype=torch.float64),
           "n_sol": torch.empty(max(Pn, 1), T, device=dev, dtype=torch.int32)}
    if return_fives:
        out["fives"] = torch.empty(max(Pn, 1), T, 5, device=dev, dtype=torch.int32)
    _lib.check(L.pram_twoview_hypotheses(_p(norm), _p(frame_off), _p(pairs), _p(match_off), _p(matches), F, Pn, M, int(first_pair), T,
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, _p(out["E"]), _p(out["n_sol"]), _p(out["fives"]) if return_fives else None,
                                         _st()), "pram_twoview_hypotheses")
    return out


def twoview_score(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, matches: torch.Tensor,
                  cam_model: torch.Tensor, cam_params: torch.Tensor, n_frames: int, n_pairs: int, n_matches: int, E: torch.Tensor,
                  n_sol: torch.Tensor, max_error: float = 4.0) -> dict:
    """E float64 [Pn, trials, TWOVIEW_MAX_SOL, 9] and n_sol int32 [Pn, trials] (twoview_hypotheses') -> h_inliers int32
    [Pn, trials, TWOVIEW_MAX_SOL] (-1 for an empty slot), h_resid float64 (same shape), best int32 [Pn] (-1: no slot)."""
    L = _lib.load()
    F, Pn, M = int(n_frames), int(n_pairs), int(n_matches)
    _twoview_views(norm, frame_off, pairs, match_off, matches, F, Pn, M)
    _twoview_cams(cam_model, cam_params, F)
    _tri_chk(((E, "E", torch.float64), (n_sol, "n_sol", torch.int32)))
    assert E.dim() == 4 and tuple(E.shape[2:]) == (TWOVIEW_MAX_SOL, 9) and E.shape[0] >= Pn and tuple(n_sol.shape) == tuple(E.shape[:2])
    T, dev = int(E.shape[1]), norm.device
    out = {"h_inliers": torch.empty(max(Pn, 1), T, TWOVIEW_MAX_SOL, device=dev, dtype=torch.int32),
           "h_resid": torch.empty(max(Pn, 1), T, TWOVIEW_MAX_SOL, device=dev, dtype=torch.float64),
           "best": torch.empty(max(Pn, 1), device=dev, dtype=torch.int32)}
    _lib.check(L.pram_twoview_score(_p(norm), _p(frame_off), _p(pairs), _p(match_off), _p(matches), _p(cam_model), _p(cam_params), F, Pn, M,
                                    _p(E), _p(n_sol), T, float(max_error), _p(out["h_inliers"]), _p(out["h_resid"]), _p(out["best"]), _st()),
               "pram_twoview_score")
    return out


_TWOVIEW_PAIR_OUT = (("E", torch.float64, (9,)), ("qvec", torch.float64, (4,)), ("tvec", torch.float64, (3,)), ("num_inliers", torch.int32, ()),
                     ("num_front", torch.int32, ()), ("success", torch.int32, ()), ("count", torch.int32, ()))
_TWOVIEW_MATCH_OUT = (("keep", torch.uint8, ()), ("kept", torch.int32, (2,)), ("edges", torch.int32, (2,)))


def twoview_outputs(n_pairs: int, n_matches: int, device) -> dict:
    """What twoview_finish writes, allocated: E float64 [Pn, 9], qvec [Pn, 4], tvec [Pn, 3], num_inliers / num_front / success /
    count int32 [Pn], and tri_verify's keep uint8 [M], kept int32 [M, 2], edges int32 [M, 2]."""
    out = {k: torch.empty(max(int(n_pairs), 1), *sh, device=device, dtype=dt) for k, dt, sh in _TWOVIEW_PAIR_OUT}
    out.update({k: torch.empty(max(int(n_matches), 1), *sh, device=device, dtype=dt) for k, dt, sh in _TWOVIEW_MATCH_OUT})
    return out


def twoview_finish(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, matches: torch.Tensor,
                   cam_model: torch.Tensor, cam_params: torch.Tensor, n_frames: int, n_pairs: int, n_matches: int, E: torch.Tensor,
                   h_inliers: torch.Tensor, best: torch.Tensor, max_error: float = 4.0, min_inlier_ratio: float = 0.1,
                   min_num_inliers: int = 15, refine_iters: int = 20, out: Optional[dict] = None) -> dict:
    """The best slot of every pair (twoview_score's) decomposed, refined and scored again -> twoview_outputs' dict.  ``out``: that
    dict with the per-pair tensors cut to this call's pairs and the per-match tensors whole (match_off indexes them), so that a
    caller walks a long pair list in chunks; None allocates it."""
    L = _lib.load()
    F, Pn, M = int(n_frames), int(n_pairs), int(n_matches)
    _twoview_views(norm, frame_off, pairs, match_off, matches, F, Pn, M)
    _twoview_cams(cam_model, cam_params, F)
    _tri_chk(((E, "E", torch.float64), (h_inliers, "h_inliers", torch.int32), (best, "best", torch.int32)))
    assert E.dim() == 4 and tuple(E.shape[2:]) == (TWOVIEW_MAX_SOL, 9) and E.shape[0] >= Pn and tuple(h_inliers.shape) == tuple(E.shape[:3])
    assert best.numel() >= Pn
    if out is None:
        out = twoview_outputs(Pn, M, norm.device)
    _tri_chk(tuple((out[k], k, dt) for k, dt, _ in _TWOVIEW_PAIR_OUT + _TWOVIEW_MATCH_OUT))
    assert all(out[k].numel() >= Pn * (sh[0] if sh else 1) for k, _, sh in _TWOVIEW_PAIR_OUT)
    assert all(out[k].numel() >= M * (sh[0] if sh else 1) for k, _, sh in _TWOVIEW_MATCH_OUT)
    _lib.check(L.pram_twoview_finish(_p(norm), _p(frame_off), _p(pairs), _p(match_off), _p(matches), _p(cam_model), _p(cam_params), F, Pn, M,
                                     _p(E), _p(h_inliers), _p(best), int(E.shape[1]), float(max_error), float(min_inlier_ratio),
                                     int(min_num_inliers), int(refine_iters), _p(out["E"]), _p(out["qvec"]), _p(out["tvec"]),
                                     _p(out["num_inliers"]), _p(out["num_front"]), _p(out["success"]), _p(out["keep"]), _p(out["kept"]),
                                     _p(out["edges"]), _p(out["count"]), _st()), "pram_twoview_finish")
    return out


# ---- statistical outlier removal (csrc/knn.hip; pram_amd/localization/outliers.py drives these) -------------------------------
KNN_TILE, KNN_MAX_K, SOR_BLOCK = 1024, 32, 1024      # include/pram_hip.h
SOR_MEAN, SOR_STD, SOR_THRESHOLD, SOR_NV = 0, 1, 2, 3      # entries of the statistics


def knn_mean_distance(x: torch.Tensor, k: int) -> torch.Tensor:
    """x float64 [n, 3] -> float64 [n]: every point's mean distance to its min(k, n) nearest points, itself included (all pairs,
    exact).  1 <= k <= KNN_MAX_K."""
    L = _lib.load()
    n = _kmeans_x(x)
    avg = torch.empty(max(n, 1), device=x.device, dtype=torch.float64)
    _lib.check(L.pram_knn_mean_distance(_p(x), n, int(k), _p(avg), _st()), "pram_knn_mean_distance")
    return avg[:n]


def sor_workspace(n: int, device) -> torch.Tensor:
    need = int(_lib.load().pram_sor_workspace_bytes(int(n)))
    if need == 0:
        raise _lib.PramHipError(f"sor_select: needs 1 <= n < 2^31, got n = {n}")
    return torch.empty(need, device=device, dtype=torch.uint8)


def sor_select(avg: torch.Tensor, std_ratio: float, workspace: Optional[torch.Tensor] = None) -> dict:
    """avg float64 [n] (:func:`knn_mean_distance`) -> stats float64 [4] (mean, std, threshold and the number of valid points, over
    the points with avg > 0), mask uint8 [n] (valid and avg < threshold), inlier_idx int32 [n] (the inliers' indices, ascending;
    the entries beyond count[0] are unspecified) and count int32 [2] (inliers, valid points).  Nothing is read back."""
    L = _lib.load()
    _chk(avg, "avg", torch.float64)
    if avg.dim() != 1 or not avg.is_contiguous():
        raise _lib.PramHipError(f"avg: expected a contiguous float64 [n] tensor, got {tuple(avg.shape)}")
    n, dev = int(avg.shape[0]), avg.device
    if workspace is None:
        workspace = sor_workspace(n, dev)
    _chk(workspace, "workspace", torch.uint8)
    out = {"stats": torch.empty(4, device=dev, dtype=torch.float64), "mask": torch.empty(max(n, 1), device=dev, dtype=torch.uint8),
           "inlier_idx": torch.empty(max(n, 1), device=dev, dtype=torch.int32), "count": torch.empty(2, device=dev, dtype=torch.int32)}
    _lib.check(L.pram_sor_select(_p(avg), n, float(std_ratio), _p(workspace), workspace.numel(), _p(out["stats"]), _p(out["mask"]),
                                 _p(out["inlier_idx"]), _p(out["count"]), _st()), "pram_sor_select")
    out["mask"], out["inlier_idx"] = out["mask"][:n], out["inlier_idx"][:n]
    return out


# ---- localisation against retrieved database frames (csrc/retrieval.hip; pram_amd/localization/retrieval.py drives these) ----
COVIS_WORKSPACE_BYTES = 64 << 20      # the histogram [n, n_frames] of one covis_topk call stays under this: longer lists go in chunks


def retr_plan(retrieval: torch.Tensor, counts: torch.Tensor, store, enable: Optional[torch.Tensor] = None) -> torch.Tensor:
    """retrieval int32 [B, n_db] (store frame indices, -1 padded), counts int32 [B], ``store``: the device tables of a DatabaseStore
    -> plan int32 [CAND_PLAN_COLS, B * n_db] whose sel_off points into valid_rows."""
    L = _lib.load()
    for t, nm in ((retrieval, "retrieval"), (counts, "counts")) + (((enable, "enable"),) if enable is not None else ()):
        _chk(t, nm, torch.int32)
        assert t.is_contiguous(), nm
    assert retrieval.dim() == 2 and counts.numel() == retrieval.shape[0] and (enable is None or enable.numel() == counts.numel())
    B, n_db = retrieval.shape
    plan = torch.empty(CAND_PLAN_COLS, B * n_db, device=retrieval.device, dtype=torch.int32)
    s = store
    _lib.check(L.pram_retr_plan(_p(retrieval), _p(counts), _p(enable), _p(s["frame_off"]), _p(s["valid_off"]), B, n_db, int(s["n_frames"]),
                                int(s["n_valid"]), _p(plan), _st()), "pram_retr_plan")
    return plan


def retr_filter(cor: dict, store, obs_th: int, out: Optional[dict] = None) -> dict:
    """cor: cand_correspond's dict -> the same lists [P, t0, ...] holding, per pair and in order, the rows whose point has obs_th
    observations or more, and their count.  ``out``: buffers to write into (the tests pre-fill them)."""
    L = _lib.load()
    P, t0 = _cor_chk(cor, "correspondences")
    if out is None:
        out = _cor_alloc(P, t0, cor["count"].device)
    else:
        assert _cor_chk(out, "out") == (P, t0)
    s = store
    _lib.check(L.pram_retr_filter(*[_p(cor[k]) for k in MATCH_KEYS], _p(cor["count"]), P, t0, _p(s["pt_ids"]), _p(s["pt_off"]), int(s["n_points"]),
                                  int(obs_th), *[_p(out[k]) for k in MATCH_KEYS], _p(out["count"]), _st()), "pram_retr_filter")
    return out


def retr_select(success: torch.Tensor, num_inliers: torch.Tensor, count: torch.Tensor, n_db: int, inlier_th: int, min_best_inliers: int) -> torch.Tensor:
    """success / num_inliers / count int32 [B * n_db] -> int32 [B, 3]: kept slot (-1 none), status (1 accepted, 2 best taken, 0
    failed), best slot (-1 none)."""
    L = _lib.load()
    for t, nm in ((success, "success"), (num_inliers, "num_inliers"), (count, "count")):
        _chk(t, nm, torch.int32)
        assert t.is_contiguous() and t.numel() == success.numel(), nm
    n_db = int(n_db)
    assert n_db >= 1 and success.numel() % n_db == 0
    B = success.numel() // n_db
    chosen = torch.empty(B, 3, device=success.device, dtype=torch.int32)
    _lib.check(L.pram_retr_select(_p(success), _p(num_inliers), _p(count), B, n_db, int(inlier_th), int(min_best_inliers), _p(chosen), _st()),
               "pram_retr_select")
    return chosen


def covis_topk(frames: torch.Tensor, store, k: int, include_self: bool = False, workspace: Optional[torch.Tensor] = None):
    """frames int32 [n] (store frame indices), ``store``: the device tables of a DatabaseStore -> (best_frames int32 [n, k] (-1
    padded), best_counts int32 [n, k], n_found int32 [n]).  workspace: int32 [>= min(n, chunk) * n_frames], dirty or not; the
    frames go through the entry in chunks whose histogram stays under COVIS_WORKSPACE_BYTES."""
    L = _lib.load()
    _chk(frames, "frames", torch.int32)
    assert frames.dim() == 1 and frames.is_contiguous()
    n, k, s, dev = frames.numel(), int(k), store, frames.device
    F = max(int(s["n_frames"]), 1)
    chunk = max(1, min(max(n, 1), COVIS_WORKSPACE_BYTES // (4 * F)))
    if workspace is None:
        workspace = torch.empty(chunk * F, device=dev, dtype=torch.int32)
    _chk(workspace, "workspace", torch.int32)
    assert workspace.is_contiguous() and workspace.numel() >= chunk * F
    best_f, best_c = torch.empty(max(n, 1), max(k, 1), device=dev, dtype=torch.int32), torch.empty(max(n, 1), max(k, 1), device=dev, dtype=torch.int32)
    n_found = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
    for a in range(0, max(n, 1), chunk):
        m = min(chunk, n - a)
        _lib.check(L.pram_covis_topk(_p(frames[a:]) if n else _p(n_found), m, _p(s["valid_off"]), _p(s["valid_rows"]), _p(s["point3D_ids"]), int(s["n_rows"]),
                                     int(s["n_valid"]), _p(s["pt_ids"]), _p(s["pt_off"]), _p(s["pt_frames"]), int(s["n_points"]), int(s["n_pt_entries"]),
                                     int(s["n_frames"]), k, int(bool(include_self)), _p(workspace), _p(best_f[a:]), _p(best_c[a:]), _p(n_found[a:]), _st()),
                   "pram_covis_topk")
    return best_f[:n], best_c[:n], n_found[:n]


# ---- bundle adjustment (csrc/bundle.hip; pram_amd/localization/bundle.py drives these) ----------------------------------------
BA_OBS_DOUBLES, BA_BLOCK, BA_CONTEXT_BYTES, BA_STATE_F64, BA_STATE_I32 = 20, 64, 512, 16, 16      # include/pram_hip.h
BA_SD_COST, BA_SD_LAM, BA_SD_COST0 = 0, 2, 9      # words of the state's float64 part
BA_SI_DONE, BA_SI_REASON, BA_SI_LM_ITER, BA_SI_ACCEPTED, BA_SI_CG_FAIL = 0, 1, 2, 3, 9      # and of its int32 part
BA_REASONS = {0: "running", 1: "max_iters", 2: "ftol", 3: "tables"}      # PRAM_BA_REASON_*
BA_STAGE_LINEARISE, BA_STAGE_BLOCKS, BA_STAGE_CG_INIT, BA_STAGE_CG, BA_STAGE_STEP, BA_STAGE_ALL = 1, 2, 4, 8, 16, 31
# the workspace's arrays in bundle.hip's order: name, dtype, columns (0: the count comes with the sizes)
BA_ARRAYS = (("table", torch.float64, "F", 16), ("table_cand", torch.float64, "F", 16), ("xyz", torch.float64, "P", 3), ("xyz_cand", torch.float64, "P", 3),
             ("jac", torch.float64, "O", 20), ("v_inv", torch.float64, "P", 6), ("g_p", torch.float64, "P", 3), ("y_p", torch.float64, "P", 3),
             ("s_block", torch.float64, "F", 21), ("diag_u", torch.float64, "F", 6), ("b", torch.float64, "F", 6), ("cg_x", torch.float64, "F", 6),
             ("cg_r", torch.float64, "F", 6), ("cg_z", torch.float64, "F", 6), ("cg_p", torch.float64, "F", 6), ("cg_q", torch.float64, "F", 6),
             ("frame_dot", torch.float64, "F2", 1), ("frame_cost", torch.float64, "F", 1), ("partials", torch.float64, "B2", 1),
             ("state_f64", torch.float64, "SD", 1), ("state_i32", torch.int32, "SI", 1), ("point_ok", torch.int32, "P", 1),
             ("moved", torch.int32, "F", 1), ("frozen", torch.int32, "F", 1), ("obs_ok", torch.uint8, "O", 1))


def ba_begin(keypoints: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor, cam_model_host, table: torch.Tensor, xyz: torch.Tensor,
             obs_row: torch.Tensor, obs_frame: torch.Tensor, obs_point: torch.Tensor, frm_off: torch.Tensor, pt_off: torch.Tensor,
             pt_obs: torch.Tensor, frozen: torch.Tensor, n_points: int, n_obs: int, n_rows: int, max_iters: int, loss_scale: float = 1.0,
             lam0: float = 1e-3, cg_tol: float = 1e-2, ftol: float = 1e-6) -> dict:
    """The problem of pram_ba_begin (include/pram_hip.h has the tables) -> a dict that holds the context, the workspace, the
    tensors the context points to (so that they outlive it) and ``views``: the workspace's arrays by BA_ARRAYS' names.  The initial
    cost is enqueued; nothing is read back."""
    import ctypes
    L = _lib.load()
    F, Pn, O, n, K = len(cam_model_host), int(n_points), int(n_obs), int(n_rows), int(max_iters)
    i32 = (("cam_model", cam_model), ("obs_row", obs_row), ("obs_frame", obs_frame), ("obs_point", obs_point), ("frm_off", frm_off),
           ("pt_off", pt_off), ("pt_obs", pt_obs), ("frozen", frozen))
    _tri_chk(((keypoints, "keypoints", torch.float32), (cam_params, "cam_params", torch.float64), (table, "table", torch.float64),
              (xyz, "xyz", torch.float64)) + tuple((t, nm, torch.int32) for nm, t in i32))
    if F < 1 or Pn < 1 or O < 1 or n < 1:
        raise _lib.PramHipError("ba_begin: needs one frame, one point, one observation and one keypoint at least")
    assert keypoints.numel() >= 2 * n and cam_model.numel() >= F and cam_params.numel() >= POSE_CAM_PARAMS * F and table.numel() >= TRI_FRAME_COLS * F
    assert xyz.numel() >= 3 * Pn and min(obs_row.numel(), obs_frame.numel(), obs_point.numel(), pt_obs.numel()) >= O
    assert frm_off.numel() >= F + 1 and pt_off.numel() >= Pn + 1 and frozen.numel() >= F
    need = int(L.pram_ba_workspace_bytes(F, Pn, O, K))
    if need == 0:
        raise _lib.PramHipError("pram_ba_begin: sizes beyond 2^24 frames, 2^28 points, 2^26 observations or 4096 iterations")
    dev = keypoints.device
    workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    offsets = (ctypes.c_size_t * (len(BA_ARRAYS) + 1))()
    _lib.check(L.pram_ba_layout(F, Pn, O, K, ctypes.addressof(offsets)), "pram_ba_layout")
    count = {"F": F, "P": Pn, "O": O, "F2": 2 * F, "B2": 2 * ((F + BA_BLOCK - 1) // BA_BLOCK), "SD": BA_STATE_F64, "SI": BA_STATE_I32 + 2 * K}
    views = {}
    for (name, dt, cnt, cols), a in zip(BA_ARRAYS, offsets):
        nbytes = count[cnt] * cols * torch.empty(0, dtype=dt).element_size()
        v = workspace[a:a + nbytes].view(dt)
        views[name] = v.view(count[cnt], cols) if cols > 1 else v
    host = _tri_models(cam_model_host, F)
    context = ctypes.create_string_buffer(BA_CONTEXT_BYTES)
    _lib.check(L.pram_ba_begin(_p(keypoints), _p(cam_model), _p(cam_params), ctypes.addressof(host), _p(table), _p(xyz), _p(obs_row), _p(obs_frame),
                               _p(obs_point), _p(frm_off), _p(pt_off), _p(pt_obs), _p(frozen), F, Pn, O, n, K, float(loss_scale), float(lam0),
                               float(cg_tol), float(ftol), _p(workspace), workspace.numel(), ctypes.addressof(context), _st()), "pram_ba_begin")
    return {"context": context, "workspace": workspace, "views": views, "n_frames": F, "n_points": Pn, "n_obs": O, "max_iters": K,
            "keep": (keypoints, cam_model, cam_params, table, xyz, obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen)}


def ba_iterate(problem: dict, n_iters: int, cg_iters: int, stages: int = BA_STAGE_ALL):
    """Enqueues n_iters Levenberg-Marquardt iterations of at most cg_iters conjugate-gradient iterations each on ``problem``
    (ba_begin's); ``stages``: BA_STAGE_* bits, for the tests and the timing tool.  Nothing is read back: the caller looks at
    problem["views"]["state_i32"][BA_SI_DONE] once per group of iterations."""
    import ctypes
    L = _lib.load()
    _lib.check(L.pram_ba_iterate(ctypes.addressof(problem["context"]), int(n_iters), int(cg_iters), int(stages), _st()), "pram_ba_iterate")


def ba_finish(problem: dict, qvec: torch.Tensor, tvec: torch.Tensor, max_reproj_error: float = 4.0, min_tri_angle: float = 0.026179938779914945) -> dict:
    """qvec float64 [F, 4], tvec float64 [F, 3]: the poses the problem's table was made from -> the refined qvec / tvec (a frame
    that never moved keeps its input bit for bit), xyz float64 [P, 3], obs_keep uint8 [O], obs_error float64 [O], pt_keep int32 [P],
    pt_error / pt_angle float64 [P], pt_kept int32 [P] and counts int32 [2] (weight-0 observations at the final state, observations
    not kept).  min_tri_angle in radians."""
    import ctypes
    L = _lib.load()
    F, Pn, O = problem["n_frames"], problem["n_points"], problem["n_obs"]
    _tri_chk(((qvec, "qvec", torch.float64), (tvec, "tvec", torch.float64)))
    assert qvec.numel() >= 4 * F and tvec.numel() >= 3 * F
    dev = qvec.device
    new = lambda m, dt, *rest: torch.empty(m, *rest, device=dev, dtype=dt)
    out = {"qvec": new(F, torch.float64, 4), "tvec": new(F, torch.float64, 3), "xyz": new(Pn, torch.float64, 3), "obs_keep": new(O, torch.uint8),
           "obs_error": new(O, torch.float64), "pt_keep": new(Pn, torch.int32), "pt_error": new(Pn, torch.float64),
           "pt_angle": new(Pn, torch.float64), "pt_kept": new(Pn, torch.int32), "counts": new(2, torch.int32)}
    _lib.check(L.pram_ba_finish(ctypes.addressof(problem["context"]), _p(qvec), _p(tvec), float(max_reproj_error), float(min_tri_angle),
                                _p(out["qvec"]), _p(out["tvec"]), _p(out["xyz"]), _p(out["obs_keep"]), _p(out["obs_error"]), _p(out["pt_keep"]),
                                _p(out["pt_error"]), _p(out["pt_angle"]), _p(out["pt_kept"]), _p(out["counts"]), _st()), "pram_ba_finish")
    return out


# ---- bundle adjustment with camera groups (csrc/bundle.hip's pram_bac_*: DESIGN.md 4.27) ---------------------------------------
BAC_OBS_DOUBLES, BAC_GROUP_PARAMS, BAC_CONTEXT_BYTES = 36, 8, 1024      # include/pram_hip.h
CAMERA_NUM_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8}      # by PRAM_CAM_* id, COLMAP's counts
# the workspace's arrays: BA_ARRAYS with rows of BAC_OBS_DOUBLES, then the groups' (G: groups, G2: 2 G, C2: 2 ceil(G / BA_BLOCK), FB: F / BA_BLOCK + G + 1)
BAC_ARRAYS = tuple((n, dt, c, BAC_OBS_DOUBLES if n == "jac" else k) for n, dt, c, k in BA_ARRAYS) + (
    ("cam_params", torch.float64, "F", 8), ("cam_params_cand", torch.float64, "F", 8), ("grp_params", torch.float64, "G", 8),
    ("grp_params_cand", torch.float64, "G", 8), ("g_block", torch.float64, "G", 36), ("g_diag_u", torch.float64, "G", 8), ("g_b", torch.float64, "G", 8),
    ("g_cg_x", torch.float64, "G", 8), ("g_cg_r", torch.float64, "G", 8), ("g_cg_z", torch.float64, "G", 8), ("g_cg_p", torch.float64, "G", 8),
    ("g_cg_q", torch.float64, "G", 8), ("group_dot", torch.float64, "G2", 1), ("g_partials", torch.float64, "C2", 1),
    ("frame_group_sums", torch.float64, "F", 60), ("frame_mv_sums", torch.float64, "F", 8), ("grp_mask", torch.int32, "G", 1),
    ("grp_bad", torch.int32, "G", 1), ("grp_model", torch.int32, "G", 1), ("fold_blocks", torch.float64, "FB", 60))


def bac_begin(keypoints: torch.Tensor, cam_model: torch.Tensor, cam_model_host, table: torch.Tensor, xyz: torch.Tensor, obs_row: torch.Tensor,
              obs_frame: torch.Tensor, obs_point: torch.Tensor, frm_off: torch.Tensor, pt_off: torch.Tensor, pt_obs: torch.Tensor,
              frozen: torch.Tensor, frm_grp: torch.Tensor, grp_off: torch.Tensor, grp_frame: torch.Tensor, grp_params: torch.Tensor,
              grp_mask: torch.Tensor, n_points: int, n_obs: int, n_rows: int, n_groups: int, max_iters: int, loss_scale: float = 1.0,
              lam0: float = 1e-3, cg_tol: float = 1e-2, ftol: float = 1e-6) -> dict:
    """The problem of pram_bac_begin: ba_begin's with camera groups in place of per-frame parameters (include/pram_hip.h has the
    tables: frm_grp int32 [F], grp_off int32 [G + 1], grp_frame int32 [F], grp_params float64 [G, 8], grp_mask int32 [G]) -> ba_begin's
    dict, ``views`` by BAC_ARRAYS' names, ``cam=True``.  The initial cost is enqueued; nothing is read back."""
    import ctypes
    L = _lib.load()
    F, Pn, O, n, G, K = len(cam_model_host), int(n_points), int(n_obs), int(n_rows), int(n_groups), int(max_iters)
    i32 = (("cam_model", cam_model), ("obs_row", obs_row), ("obs_frame", obs_frame), ("obs_point", obs_point), ("frm_off", frm_off),
           ("pt_off", pt_off), ("pt_obs", pt_obs), ("frozen", frozen), ("frm_grp", frm_grp), ("grp_off", grp_off), ("grp_frame", grp_frame),
           ("grp_mask", grp_mask))
    _tri_chk(((keypoints, "keypoints", torch.float32), (grp_params, "grp_params", torch.float64), (table, "table", torch.float64),
              (xyz, "xyz", torch.float64)) + tuple((t, nm, torch.int32) for nm, t in i32))
    if F < 1 or Pn < 1 or O < 1 or n < 1 or G < 1 or G > F:
        raise _lib.PramHipError("bac_begin: needs one frame, one point, one observation and one keypoint at least, and 1 <= groups <= frames")
    assert keypoints.numel() >= 2 * n and cam_model.numel() >= F and table.numel() >= TRI_FRAME_COLS * F
    assert xyz.numel() >= 3 * Pn and min(obs_row.numel(), obs_frame.numel(), obs_point.numel(), pt_obs.numel()) >= O
    assert frm_off.numel() >= F + 1 and pt_off.numel() >= Pn + 1 and frozen.numel() >= F
    assert frm_grp.numel() >= F and grp_frame.numel() >= F and grp_off.numel() >= G + 1 and grp_params.numel() >= BAC_GROUP_PARAMS * G and grp_mask.numel() >= G
    need = int(L.pram_bac_workspace_bytes(F, Pn, O, G, K))
    if need == 0:
        raise _lib.PramHipError("pram_bac_begin: sizes beyond 2^24 frames, 2^28 points, 2^26 observations or 4096 iterations")
    dev = keypoints.device
    workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    offsets = (ctypes.c_size_t * (len(BAC_ARRAYS) + 1))()
    _lib.check(L.pram_bac_layout(F, Pn, O, G, K, ctypes.addressof(offsets)), "pram_bac_layout")
    count = {"F": F, "P": Pn, "O": O, "F2": 2 * F, "B2": 2 * ((F + BA_BLOCK - 1) // BA_BLOCK), "SD": BA_STATE_F64, "SI": BA_STATE_I32 + 2 * K,
             "G": G, "G2": 2 * G, "C2": 2 * ((G + BA_BLOCK - 1) // BA_BLOCK), "FB": F // BA_BLOCK + G + 1}
    views = {}
    for (name, dt, cnt, cols), a in zip(BAC_ARRAYS, offsets):
        nbytes = count[cnt] * cols * torch.empty(0, dtype=dt).element_size()
        v = workspace[a:a + nbytes].view(dt)
        views[name] = v.view(count[cnt], cols) if cols > 1 else v
    host = _tri_models(cam_model_host, F)
    context = ctypes.create_string_buffer(BAC_CONTEXT_BYTES)
    _lib.check(L.pram_bac_begin(_p(keypoints), _p(cam_model), ctypes.addressof(host), _p(table), _p(xyz), _p(obs_row), _p(obs_frame), _p(obs_point),
                                _p(frm_off), _p(pt_off), _p(pt_obs), _p(frozen), _p(frm_grp), _p(grp_off), _p(grp_frame), _p(grp_params),
                                _p(grp_mask), F, Pn, O, n, G, K, float(loss_scale), float(lam0), float(cg_tol), float(ftol), _p(workspace),
                                workspace.numel(), ctypes.addressof(context), _st()), "pram_bac_begin")
    return {"context": context, "workspace": workspace, "views": views, "n_frames": F, "n_points": Pn, "n_obs": O, "n_groups": G, "max_iters": K,
            "cam": True, "keep": (keypoints, cam_model, table, xyz, obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen, frm_grp,
                                  grp_off, grp_frame, grp_params, grp_mask)}


def bac_iterate(problem: dict, n_iters: int, cg_iters: int, stages: int = BA_STAGE_ALL):
    """ba_iterate on a problem of bac_begin."""
    import ctypes
    L = _lib.load()
    _lib.check(L.pram_bac_iterate(ctypes.addressof(problem["context"]), int(n_iters), int(cg_iters), int(stages), _st()), "pram_bac_iterate")


def bac_finish(problem: dict, qvec: torch.Tensor, tvec: torch.Tensor, max_reproj_error: float = 4.0, min_tri_angle: float = 0.026179938779914945) -> dict:
    """ba_finish on a problem of bac_begin, evaluated with the refined parameters, and ``grp_params`` float64 [G, 8]: the refined
    parameters (a group that never moved keeps its input bit for bit)."""
    import ctypes
    L = _lib.load()
    F, Pn, O, G = problem["n_frames"], problem["n_points"], problem["n_obs"], problem["n_groups"]
    _tri_chk(((qvec, "qvec", torch.float64), (tvec, "tvec", torch.float64)))
    assert qvec.numel() >= 4 * F and tvec.numel() >= 3 * F
    dev = qvec.device
    new = lambda m, dt, *rest: torch.empty(m, *rest, device=dev, dtype=dt)
    out = {"qvec": new(F, torch.float64, 4), "tvec": new(F, torch.float64, 3), "xyz": new(Pn, torch.float64, 3), "obs_keep": new(O, torch.uint8),
           "obs_error": new(O, torch.float64), "pt_keep": new(Pn, torch.int32), "pt_error": new(Pn, torch.float64),
           "pt_angle": new(Pn, torch.float64), "pt_kept": new(Pn, torch.int32), "counts": new(2, torch.int32),
           "grp_params": new(G, torch.float64, BAC_GROUP_PARAMS)}
    _lib.check(L.pram_bac_finish(ctypes.addressof(problem["context"]), _p(qvec), _p(tvec), float(max_reproj_error), float(min_tri_angle),
                                 _p(out["qvec"]), _p(out["tvec"]), _p(out["xyz"]), _p(out["obs_keep"]), _p(out["obs_error"]), _p(out["pt_keep"]),
                                 _p(out["pt_error"]), _p(out["pt_angle"]), _p(out["pt_kept"]), _p(out["counts"]), _p(out["grp_params"]), _st()),
               "pram_bac_finish")
    return out


# ---- incremental mapping (csrc/mapper.hip; pram_amd/localization/mapper.py drives these) --------------------------------------
MAP_MAX_LINKS = 8      # PRAM_MAP_MAX_LINKS


def map_pair_angles(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, kept: torch.Tensor,
                    count: torch.Tensor, qvec: torch.Tensor, tvec: torch.Tensor, success: torch.Tensor, n_frames: int, n_pairs: int,
                    n_matches: int, workspace: Optional[torch.Tensor] = None) -> dict:
    """norm: tri_normalize with offset 0.5; pairs / match_off: the match CSR; kept int32 [M, 2], count, qvec [Pn, 4], tvec [Pn, 3],
    success int32 [Pn]: twoview_finish's -> n_tri int32 [Pn] (the kept matches whose midpoint lies in front of both cameras) and
    tri_angle float64 [Pn] (the lower median of their angles, radians; 0 for n_tri = 0)."""
    L = _lib.load()
    F, Pn, M = int(n_frames), int(n_pairs), int(n_matches)
    _twoview_views(norm, frame_off, pairs, match_off, kept, F, Pn, M)
    _tri_chk(((count, "count", torch.int32), (qvec, "qvec", torch.float64), (tvec, "tvec", torch.float64), (success, "success", torch.int32)))
    assert count.numel() >= Pn and qvec.numel() >= 4 * Pn and tvec.numel() >= 3 * Pn and success.numel() >= Pn
    dev = norm.device
    workspace = _tri_workspace(int(L.pram_map_pair_angles_workspace_bytes(M)), "pram_map_pair_angles: a negative number of matches", workspace, dev)
    out = {"n_tri": torch.empty(max(Pn, 1), device=dev, dtype=torch.int32), "tri_angle": torch.empty(max(Pn, 1), device=dev, dtype=torch.float64)}
    _lib.check(L.pram_map_pair_angles(_p(norm), _p(frame_off), _p(pairs), _p(match_off), _p(kept), _p(count), _p(qvec), _p(tvec), _p(success),
                                      F, Pn, M, _p(workspace), workspace.numel(), _p(out["n_tri"]), _p(out["tri_angle"]), _st()),
               "pram_map_pair_angles")
    return out


def map_seed(success: torch.Tensor, n_tri: torch.Tensor, tri_angle: torch.Tensor, n_pairs: int, min_num_inliers: int,
             min_tri_angle: float) -> torch.Tensor:
    """-> int32 [1]: the eligible pair (success, n_tri >= min_num_inliers, tri_angle >= min_tri_angle in radians) with the largest
    n_tri, the lowest position on a tie; -1 when none is eligible.  On the device."""
    L = _lib.load()
    Pn = int(n_pairs)
    _tri_chk(((success, "success", torch.int32), (n_tri, "n_tri", torch.int32), (tri_angle, "tri_angle", torch.float64)))
    assert success.numel() >= Pn and n_tri.numel() >= Pn and tri_angle.numel() >= Pn
    seed = torch.empty(1, device=success.device, dtype=torch.int32)
    _lib.check(L.pram_map_seed(_p(success), _p(n_tri), _p(tri_angle), Pn, int(min_num_inliers), float(min_tri_angle), _p(seed), _st()),
               "pram_map_seed")
    return seed


def map_correspond(adj_off: torch.Tensor, adj: torch.Tensor, row_frame: torch.Tensor, n_adj: int, frame_off: torch.Tensor,
                   registered: torch.Tensor, row_point: torch.Tensor, n_frames: int, n_rows: int, n_points: int,
                   capacity: Optional[int] = None) -> dict:
    """adj_off / adj / row_frame: tri_adjacency's (n_adj: the entries adj holds); registered uint8 [F]; row_point int32 [n_rows]
    -> n_corr int32 [F], corr_off int32 [F + 1], dropped int32 [F], corr_row / corr_point int32 [capacity] ordered by (row, point).
    capacity: None sizes the lists for the worst case, min(MAP_MAX_LINKS * n_rows, n_adj)."""
    L = _lib.load()
    F, n, A, Pt = int(n_frames), int(n_rows), int(n_adj), int(n_points)
    _tri_chk(((adj_off, "adj_off", torch.int32), (adj, "adj", torch.int32), (row_frame, "row_frame", torch.int32), (frame_off, "frame_off", torch.int32),
              (registered, "registered", torch.uint8), (row_point, "row_point", torch.int32)))
    assert adj_off.numel() >= n + 1 and adj.numel() >= A and row_frame.numel() >= n and frame_off.numel() >= F + 1
    assert registered.numel() >= F and row_point.numel() >= n
    cap = min(MAP_MAX_LINKS * n, A) if capacity is None else int(capacity)
    dev = adj.device
    i32 = lambda m: torch.empty(max(m, 1), device=dev, dtype=torch.int32)
    out = {"n_corr": i32(F), "corr_off": i32(F + 1), "dropped": i32(F), "corr_row": i32(cap), "corr_point": i32(cap), "capacity": cap}
    _lib.check(L.pram_map_correspond(_p(adj_off), _p(adj), _p(row_frame), A, _p(frame_off), _p(registered), _p(row_point), F, n, Pt, cap,
                                     _p(out["n_corr"]), _p(out["corr_off"]), _p(out["dropped"]), _p(out["corr_row"]), _p(out["corr_point"]), _st()),
               "pram_map_correspond")
    return out


def map_choose(n_corr: torch.Tensor, registered: torch.Tensor, tries: torch.Tensor, n_frames: int, min_corr: int = 30, max_reg_trials: int = 3,
               round_frames: int = 0) -> dict:
    """-> chosen int32 [F] (-1 padded), chosen_count int32 [F] and n_chosen int32 [1], on the device: the unregistered frames with
    n_corr >= min_corr and tries < max_reg_trials by (n_corr descending, frame ascending), round_frames of them at most (0: all)."""
    L = _lib.load()
    F = int(n_frames)
    _tri_chk(((n_corr, "n_corr", torch.int32), (registered, "registered", torch.uint8), (tries, "tries", torch.int32)))
    assert n_corr.numel() >= F and registered.numel() >= F and tries.numel() >= F
    i32 = lambda m: torch.empty(max(m, 1), device=n_corr.device, dtype=torch.int32)
    out = {"chosen": i32(F), "chosen_count": i32(F), "n_chosen": i32(1)}
    _lib.check(L.pram_map_choose(_p(n_corr), _p(registered), _p(tries), F, int(min_corr), int(max_reg_trials), int(round_frames), _p(out["chosen"]),
                                 _p(out["chosen_count"]), _p(out["n_chosen"]), _st()), "pram_map_choose")
    return out


def map_pack(chosen: torch.Tensor, n_chosen: int, corr: dict, keypoints: torch.Tensor, xyz: torch.Tensor, n_frames: int, n_rows: int,
             n_points: int, t0: int) -> dict:
    """chosen int32 [S]; corr: map_correspond's dict -> matched_keypoints float32 [S, t0, 2], matched_xyzs float64 [S, t0, 3], counts
    int32 [S] and cut int32 [S] (the rows beyond t0), as pose.estimate_poses takes them."""
    L = _lib.load()
    S, F, n, Pt, t0 = int(n_chosen), int(n_frames), int(n_rows), int(n_points), int(t0)
    _tri_chk(((chosen, "chosen", torch.int32), (corr["corr_off"], "corr_off", torch.int32), (corr["corr_row"], "corr_row", torch.int32),
              (corr["corr_point"], "corr_point", torch.int32), (keypoints, "keypoints", torch.float32), (xyz, "xyz", torch.float64)))
    cap = int(corr["capacity"])
    assert chosen.numel() >= S and corr["corr_off"].numel() >= F + 1 and min(corr["corr_row"].numel(), corr["corr_point"].numel()) >= cap
    assert keypoints.numel() >= 2 * n and xyz.numel() >= 3 * Pt
    dev = chosen.device
    out = {"matched_keypoints": torch.empty(max(S, 1), max(t0, 1), 2, device=dev, dtype=torch.float32),
           "matched_xyzs": torch.empty(max(S, 1), max(t0, 1), 3, device=dev, dtype=torch.float64),
           "counts": torch.empty(max(S, 1), device=dev, dtype=torch.int32), "cut": torch.empty(max(S, 1), device=dev, dtype=torch.int32)}
    _lib.check(L.pram_map_pack(_p(chosen), S, _p(corr["corr_off"]), _p(corr["corr_row"]), _p(corr["corr_point"]), cap, _p(keypoints), _p(xyz), F, n,
                               Pt, t0, _p(out["matched_keypoints"]), _p(out["matched_xyzs"]), _p(out["counts"]), _p(out["cut"]), _st()),
               "pram_map_pack")
    return out


def map_live_edges(edges: torch.Tensor, n_edges: int, row_frame: torch.Tensor, registered: torch.Tensor, n_frames: int, n_rows: int) -> torch.Tensor:
    """edges int32 [n_edges, 2] rows -> int32 [n_edges, 2]: the edge where the frames of both ends are registered, (-1, -1) elsewhere."""
    L = _lib.load()
    m, F, n = int(n_edges), int(n_frames), int(n_rows)
    _tri_chk(((edges, "edges", torch.int32), (row_frame, "row_frame", torch.int32), (registered, "registered", torch.uint8)))
    assert edges.numel() >= 2 * m and row_frame.numel() >= n and registered.numel() >= F
    out = torch.empty(max(m, 1), 2, device=edges.device, dtype=torch.int32)
    _lib.check(L.pram_map_live_edges(_p(edges), m, _p(row_frame), _p(registered), F, n, _p(out), _st()), "pram_map_live_edges")
    return out


# ---- image retrieval (csrc/imgret.hip; pram_amd/localization/image_retrieval.py drives these) --------------------------------
IMGRET_DIM, IMGRET_MAX_K, IMGRET_MAX_TOPK, IMGRET_MAX_SPLITS = 128, 256, 64, 1024      # include/pram_hip.h
IMGRET_QUERY_TILE, IMGRET_DB_TILE = 32, 128      # the tile of pram_imgret_topk's grid: what a choice of ``splits`` starts from


def _imgret_rows(t: torch.Tensor, name: str) -> int:
    _chk(t, name)
    if t.dim() != 2 or t.shape[1] != IMGRET_DIM or not t.is_contiguous():
        raise _lib.PramHipError(f"{name}: expected a contiguous float32 [n, {IMGRET_DIM}] tensor, got {tuple(t.shape)}")
    return int(t.shape[0])


def imgret_assign(desc: torch.Tensor, centres: torch.Tensor):
    """desc float32 [n, 128], centres float32 [k, 128] -> (labels int32 [n]: the nearest centre, the lowest index on a tie, dist
    float64 [n]: its squared distance, summed in float64 over ascending d)."""
    L = _lib.load()
    n, k = _imgret_rows(desc, "desc"), _imgret_rows(centres, "centres")
    labels = torch.empty(max(n, 1), device=desc.device, dtype=torch.int32)
    dist = torch.empty(max(n, 1), device=desc.device, dtype=torch.float64)
    _lib.check(L.pram_imgret_assign(_p(desc), n, _p(centres), k, _p(labels), _p(dist), _st()), "pram_imgret_assign")
    return labels[:n], dist[:n]


def imgret_aggregate(desc: torch.Tensor, labels: torch.Tensor, centres: torch.Tensor, first: torch.Tensor, count: torch.Tensor):
    """The residual sums of the images first[i] .. first[i] + count[i] - 1 (int32 [n_img] row ranges into desc) -> (sums float64
    [n_img, k, 128]: per centre the sum of x - c over the image's rows with that label in ascending row index, n_assigned int32
    [n_img, k])."""
    L = _lib.load()
    n, k = _imgret_rows(desc, "desc"), _imgret_rows(centres, "centres")
    _tri_chk(((labels, "labels", torch.int32), (first, "first", torch.int32), (count, "count", torch.int32)))
    assert labels.numel() >= n and first.dim() == 1 and count.numel() == first.numel()
    m = first.numel()
    sums = torch.empty(max(m, 1), max(k, 1), IMGRET_DIM, device=desc.device, dtype=torch.float64)
    n_assigned = torch.empty(max(m, 1), max(k, 1), device=desc.device, dtype=torch.int32)
    _lib.check(L.pram_imgret_aggregate(_p(desc), _p(labels), n, _p(centres), k, _p(first), _p(count), m, _p(sums), _p(n_assigned), _st()),
               "pram_imgret_aggregate")
    return sums[:m], n_assigned[:m]


def imgret_fold(sums: torch.Tensor, n_assigned: torch.Tensor, total: torch.Tensor, total_n: torch.Tensor) -> None:
    """Adds the blocks' sums float64 [n_blk, k, 128] and n_assigned int32 [n_blk, k] onto total float64 [k, 128] and total_n int32
    [k], in ascending block order."""
    L = _lib.load()
    _tri_chk(((sums, "sums", torch.float64), (n_assigned, "n_assigned", torch.int32), (total, "total", torch.float64), (total_n, "total_n", torch.int32)))
    k = int(total_n.numel())
    assert sums.dim() == 3 and sums.shape[1] == k and sums.shape[2] == IMGRET_DIM and n_assigned.numel() == sums.shape[0] * k and total.numel() == k * IMGRET_DIM
    _lib.check(L.pram_imgret_fold(_p(sums), _p(n_assigned), int(sums.shape[0]), k, _p(total), _p(total_n), _st()), "pram_imgret_fold")


def imgret_update(centres: torch.Tensor, total: torch.Tensor, total_n: torch.Tensor) -> None:
    """centres float32 [k, 128] in place: c <- float(double(c) + total / total_n) where total_n > 0."""
    L = _lib.load()
    k = _imgret_rows(centres, "centres")
    _tri_chk(((total, "total", torch.float64), (total_n, "total_n", torch.int32)))
    assert total.numel() == k * IMGRET_DIM and total_n.numel() == k
    _lib.check(L.pram_imgret_update(_p(centres), _p(total), _p(total_n), k, _st()), "pram_imgret_update")


def imgret_normalize(sums: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sums float64 [n_img, k, 128] -> the VLAD vectors float32 [n_img, k * 128] (into ``out`` when given): every centre's block
    divided by its norm, then the whole by its norm; an image without rows is all zeros."""
    L = _lib.load()
    _chk(sums, "sums", torch.float64)
    if sums.dim() != 3 or sums.shape[2] != IMGRET_DIM or not sums.is_contiguous():
        raise _lib.PramHipError(f"sums: expected a contiguous float64 [n_img, k, {IMGRET_DIM}] tensor, got {tuple(sums.shape)}")
    m, k = int(sums.shape[0]), int(sums.shape[1])
    if out is None:
        out = torch.empty(max(m, 1), max(k, 1) * IMGRET_DIM, device=sums.device, dtype=torch.float32)
    _chk(out, "out")
    assert out.is_contiguous() and out.numel() >= m * k * IMGRET_DIM
    _lib.check(L.pram_imgret_normalize(_p(sums), m, k, _p(out), _st()), "pram_imgret_normalize")
    return out[:m]


def imgret_topk(q: torch.Tensor, db: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None, db_valid: Optional[torch.Tensor] = None,
                splits: int = 1, workspace: Optional[torch.Tensor] = None):
    """q float32 [nq, L], db float32 [nd, L] (L a multiple of 128) -> (idx int32 [nq, k], sim float32 [nq, k]): per query the k
    database rows of largest inner product (exact fp32, one chain over L), similarity descending, then index ascending; -1 / 0 where
    fewer are allowed.  exclude int32 [nq]: an index the query may not return (-1 none); db_valid uint8 [nd]: 0 bars a row.  The
    result is the same bits for every ``splits``."""
    L_ = _lib.load()
    _chk(q, "q"), _chk(db, "db")
    if q.dim() != 2 or db.dim() != 2 or q.shape[1] != db.shape[1] or not q.is_contiguous() or not db.is_contiguous():
        raise _lib.PramHipError(f"imgret_topk: expected contiguous float32 [nq, L] and [nd, L], got {tuple(q.shape)} and {tuple(db.shape)}")
    nq, nd, Ln, k, splits = int(q.shape[0]), int(db.shape[0]), int(q.shape[1]), int(k), int(splits)
    if exclude is not None:
        _chk(exclude, "exclude", torch.int32)
        assert exclude.is_contiguous() and exclude.numel() >= nq
    if db_valid is not None:
        _chk(db_valid, "db_valid", torch.uint8)
        assert db_valid.is_contiguous() and db_valid.numel() >= nd
    need = int(L_.pram_imgret_topk_workspace_bytes(nq, k, splits))
    if workspace is None:
        workspace = _workspace(need, q.device, "imgret_topk")
    _chk(workspace, "workspace", torch.uint8)
    idx = torch.empty(max(nq, 1), max(k, 1), device=q.device, dtype=torch.int32)
    sim = torch.empty(max(nq, 1), max(k, 1), device=q.device, dtype=torch.float32)
    _lib.check(L_.pram_imgret_topk(_p(q), nq, _p(db), nd, Ln, _p(exclude), _p(db_valid), k, splits, _p(workspace), workspace.numel(), _p(idx),
                                   _p(sim), _st()), "pram_imgret_topk")
    return idx[:nq], sim[:nq]
