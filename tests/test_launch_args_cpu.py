"""Argument checks of the GEMM and convolution entries of the C ABI, one invalid argument at a time (no GPU: nothing launches).

Every row calls an entry with an EMPTY problem (m = 0 for the linear entries, batch = 0 for conv and bgemm) and otherwise
valid-looking arguments, non-null integers as pointers.  The checks run before the empty-problem return, so a caught argument
comes back as PRAM_E_ARG (-1) and a missed one as 0 — whatever the code under test does, no kernel is launched and no pointer
is followed.  The message in pram_last_error must name the entry that was CALLED (the shared implementations behind several
entries once reported all of them as pram_linear_x3_f32 / pram_linear_f32) and say what is wrong."""
import pytest

from pram_amd import _lib

P = 0x1000      # a non-null "pointer": never dereferenced, the problem is empty


def _spec(text):
    """'a0=P lda0=64 alpha=1.0' -> ordered dict; P = pointer, a dot makes a float"""
    out = {}
    for item in text.split():
        k, v = item.split("=")
        out[k] = P if v == "P" else (float(v) if "." in v else int(v))
    return out


_ROT = "flags=0 rot_cos=0 rot_sin=0 rot_cols=0"
_A = "a0=P lda0=64 k0=64 a1=0 lda1=0 k1=0"
_X3 = _A + " w_hi=P w_lo=P w_scale=1.0 bias=0 residual=0 ldr=0 out=P ldo=128 out_hi=0 out_lo=0 ldo16=0 m=0 n=128 alpha=1.0 " + _ROT
_F16 = _A + " w=P bias=0 residual=0 ldr=0 out=P ldo=128 m=0 n=128 alpha=1.0 " + _ROT
_CONV = "in=P batch=0 h=32 w=32 cin=64 wgt=P bias=0 scale=0 shift=0 residual=0 out=P cout=64 ks=3 stride=1 relu=0 stream=0"
_CONVX3 = "in=P batch=0 h=32 w=32 cin=64 wgt_hi=P wgt_lo=P w_scale=1.0 bias=0 scale=0 shift=0 residual=0 out=P cout=64 ks=3 stride=1 relu=0 stream=0"

BASE = {
    "pram_linear_x3p_f32": _spec("a0_hi=P a0_lo=P lda0=64 k0=64 a1_hi=0 a1_lo=0 lda1=0 k1=0 w_hi=P w_lo=P w_scale=1.0 bias=0 residual=0 ldr=0 "
                                 "out=P ldo=128 out_hi=0 out_lo=0 ldo16=0 m=0 n=128 alpha=1.0 " + _ROT + " stream=0"),
    "pram_linear_x3_f32": _spec(_X3 + " stream=0"),
    "pram_linear_x3_ragged_f32": _spec(_X3 + " lens=0 t_pad=0 stream=0"),
    "pram_linear_x3_ssq_f32": _spec(_A + " w_hi=P w_lo=P w_scale=1.0 bias=0 out=P ldo=128 row_ssq=P m=0 n=128 lens=0 t_pad=0 stream=0"),
    "pram_linear_x3_lngelu_f32": _spec("hidden=P ldh=64 k=64 w_hi=P w_lo=P w_scale=1.0 bias=0 residual=0 ldr=0 out=P ldo=128 m=0 n=128 "
                                       "ln_ssq=P parts=1 gamma=P beta=P eps=0.00001 lens=0 t_pad=0 stream=0"),
    "pram_linear_x3_qkv_f32": _spec("a0=P lda0=64 k0=64 w_hi=P w_lo=P w_scale=1.0 bias=0 out_hi=P out_lo=P ldo16=128 vt_hi=P vt_lo=P vt_col0=128 "
                                    "heads=1 t_seq=64 m=0 n=192 " + _ROT + " lens=0 stream=0"),
    "pram_linear_f16_f32": _spec(_F16 + " stream=0"),
    "pram_linear_f16_ragged_f32": _spec(_F16 + " lens=0 t_pad=0 stream=0"),
    "pram_linear_f16_h16": _spec(_A + " w=P bias=0 residual=0 ldr=0 out=P ldo=128 out16=P ldo16=128 m=0 n=128 alpha=1.0 " + _ROT + " stream=0"),
    "pram_linear_f32": _spec(_F16 + " stream=0"),
    "pram_linear_ragged_f32": _spec(_F16 + " lens=0 t_pad=0 stream=0"),
    "pram_bgemm_nt_f32": _spec("a=P lda=64 stride_a=0 b=P ldb=64 stride_b=0 c=P ldc=64 stride_c=0 batch=0 m_max=64 n_max=64 k=64 alpha=1.0 stream=0"),
    "pram_bgemm_nt_x3p_f32": _spec("a_hi=P a_lo=P lda=64 stride_a=0 b_hi=P b_lo=P ldb=64 stride_b=0 c=P ldc=64 stride_c=0 batch=0 m_max=64 "
                                   "n_max=64 k=64 alpha=1.0 stream=0"),
    "pram_conv2d_nhwc_f32": _spec(_CONV),
    "pram_conv2d_nhwc_f16_f32": _spec(_CONV),
    "pram_conv2d_nhwc_x3_f32": _spec(_CONVX3),
    "pram_conv2d_nhwc_x3_l2norm_f32": _spec(_CONVX3),
    "pram_conv2d_nhwc_x3_planes": _spec(_CONVX3.replace("out=P", "out_hi=P out_lo=P")),
}

_CAT = "a1=P lda1=64"                       # a second input segment (k0 / k1 given per row)
_LENS0 = ("lens=P t_pad=0", "lens needs t_pad > 0")
_ROTARY = ("flags=1", "rotary needs cos/sin")
_ONE_PLANE = ("out_hi=P", "the split output needs both planes")
_HUGE = "h=8192 w=8192 cin=64"              # 2^32 elements per image: beyond the loaders' 32-bit offsets
_CONV_COMMON = [("in=0", "null pointer"), ("ks=2", "ks must be 1 or 3"), ("stride=3", "stride must be 1 or 2"),
                ("scale=P", "scale and shift go together")]
_CONV_OFFSETS = _CONV_COMMON + [(_HUGE, "does not fit the 32-bit offsets")]

# entry -> [(overrides of ONE argument (with what it needs to be reached), expected substring of the message)]
INVALID = {
    "pram_linear_x3p_f32": [("a0_lo=0", "null pointer"), ("k0=48", "k0, k1 must be multiples of 32"), ("lda0=60", "lda of 8"),
                            ("a1_hi=P lda1=64 k1=32", "second segment needs both planes"), _ROTARY, _ONE_PLANE],
    "pram_linear_x3_f32": [("a0=0", "null pointer"), ("k0=60", "K must be a multiple of 8"), ("lda0=62", "lda of 4"),
                           (_CAT + " k0=48 k1=16", "concat needs k0 % 32 == 0"), _ROTARY, _ONE_PLANE],
    "pram_linear_x3_ragged_f32": [("w_lo=0", "null pointer"), ("k0=60", "K must be a multiple of 8"),
                                  (_CAT + " k0=48 k1=16", "concat needs k0 % 32 == 0"), _ROTARY, _LENS0, _ONE_PLANE],
    "pram_linear_x3_ssq_f32": [("row_ssq=0", "null pointer"), ("a0=0", "null pointer"), ("k0=60", "K must be a multiple of 8"),
                               (_CAT + " k0=48 k1=16", "concat needs k0 % 32 == 0"), _LENS0],
    "pram_linear_x3_lngelu_f32": [("ln_ssq=0", "null pointer"), ("hidden=0", "null pointer"), ("n=64", "must exceed 64"),
                                  ("k=1056 ldh=1056", "K <= 1024"), ("k=40 ldh=40", "K % 32 == 0"), ("gamma=0", "needs gamma / beta / parts"), _LENS0],
    "pram_linear_x3_qkv_f32": [("a0=0", "null pointer"), ("vt_hi=0", "null pointer"), ("out_lo=0", "null pointer"), ("k0=60", "K must be a multiple of 8"),
                               ("t_seq=48", "multiple of 64 tokens"), ("vt_col0=64", "value heads must be the last"), _ROTARY],
    "pram_linear_f16_f32": [("w=0", "null pointer"), ("k0=60", "K must be a multiple of 8"), (_CAT + " k0=32 k1=32", "concat needs k0 % 64 == 0"), _ROTARY],
    "pram_linear_f16_ragged_f32": [("out=0", "null pointer"), ("lda0=62", "lda of 4"), (_CAT + " k0=32 k1=32", "concat needs k0 % 64 == 0"),
                                   _ROTARY, _LENS0],
    "pram_linear_f16_h16": [("out16=0", "null pointer"), ("a0=0", "null pointer"), ("k0=60", "K must be a multiple of 8"),
                            (_CAT + " k0=32 k1=32", "concat needs k0 % 64 == 0"), _ROTARY],
    "pram_linear_f32": [("a0=0", "null pointer"), ("k0=62", "K and lda must be multiples of 4"), ("n=0", "bad sizes m=0 n=0 k0=64 k1=0"),
                        (_CAT + " k0=48 k1=16", "concat needs k0 % 32 == 0"), _ROTARY],
    "pram_linear_ragged_f32": [("w=0", "null pointer"), ("lda0=62", "K and lda must be multiples of 4"),
                               (_CAT + " k0=48 k1=16", "concat needs k0 % 32 == 0"), _ROTARY, _LENS0],
    "pram_bgemm_nt_f32": [("b=0", "null pointer"), ("k=62 ldb=62", "need k % 4 == 0"), ("ldb=32", "ldb == k")],
    "pram_bgemm_nt_x3p_f32": [("b_lo=0", "null pointer"), ("k=48 ldb=48", "need k % 32 == 0"), ("stride_a=4", "plane strides % 8 == 0")],
    "pram_conv2d_nhwc_f32": _CONV_COMMON + [("cin=8", "must be 4 or a multiple of 32")],
    "pram_conv2d_nhwc_f16_f32": _CONV_OFFSETS + [("cin=32", "must be a multiple of 64")],
    "pram_conv2d_nhwc_x3_f32": _CONV_OFFSETS + [("cin=16", "must be a multiple of 32"), ("wgt_lo=0", "null pointer")],
    "pram_conv2d_nhwc_x3_l2norm_f32": _CONV_OFFSETS + [("cin=16", "must be a multiple of 32"), ("cout=256", "must be at most 128")],
    "pram_conv2d_nhwc_x3_planes": _CONV_OFFSETS + [("cin=16", "must be a multiple of 32"), ("cout=63", "must be even"), ("out_lo=0", "null pointer")],
}

# valid variations that must stay valid: optional arguments, and the one entry without the 32-bit offset bound
VALID = [("pram_linear_f16_h16", "out=0"), ("pram_linear_x3_f32", "out=0 out_hi=P out_lo=P ldo16=128"), ("pram_conv2d_nhwc_f32", _HUGE),
         ("pram_conv2d_nhwc_f32", "cin=4"), ("pram_linear_x3_ragged_f32", "lens=P t_pad=64"), ("pram_linear_x3_qkv_f32", "lens=P")]


def _call(entry, overrides):
    args = dict(BASE[entry])
    for k, v in _spec(overrides).items():
        assert k in args, (entry, k)
        args[k] = v
    L = _lib.load()
    assert len(args) == len(_lib._SIGS[entry][1]), entry
    rc = getattr(L, entry)(*args.values())
    return rc, (L.pram_last_error() or b"").decode()


def test_the_table_covers_every_linear_and_conv2d_entry():
    want = {n for n in _lib._SIGS if (n.startswith(("pram_linear_", "pram_bgemm_nt_", "pram_conv2d_nhwc_")) and n != "pram_linear_x3_ssq_parts")}
    assert want == set(BASE) == set(INVALID)


@pytest.mark.parametrize("entry", sorted(BASE))
def test_valid_arguments_and_an_empty_problem_return_ok(entry):
    rc, msg = _call(entry, "")
    assert rc == 0, (entry, rc, msg)


@pytest.mark.parametrize("entry,overrides", VALID)
def test_optional_arguments_stay_optional(entry, overrides):
    rc, msg = _call(entry, overrides)
    assert rc == 0, (entry, overrides, rc, msg)


@pytest.mark.parametrize("entry,overrides,expect", [(e, o, x) for e in sorted(INVALID) for o, x in INVALID[e]])
def test_one_invalid_argument_is_refused_by_name(entry, overrides, expect):
    rc, msg = _call(entry, overrides)
    assert rc == -1, (entry, overrides, rc, msg)
    assert expect in msg, (entry, overrides, msg)
    assert msg.startswith(entry + ":"), (entry, overrides, msg)
