"""Which kernel instantiation every size-dependent launch site can pick, and one or more cases that reach each of them.

The GEMM, convolution and split-fp16 attention entries choose their instantiation from the launch grid (gemm::choose_tile in
csrc/gemm_core.h, launch_linear_x3_wide / launch_linear_split / launch_linear / launch_linear_f16 in csrc/linear.hip, the
pram_conv2d_nhwc_* entries in csrc/conv.hip, pram_attention_x3_f32 / launch_h16t in csrc/attention_x3.hip).  Every such site
records what it launched (PRAM_NOTE_LAUNCH in csrc/launch.h; ops.last_kernel() reads it).  This file is written by hand from
that dispatch code:

  FAMILIES  family literal of PRAM_NOTE_LAUNCH -> {tag: the rule that selects it}
  BARS      the absolute error bars, each quoted from the existing test of that path
  CASES     entry, shape, options and the tag the case must land on

tests/test_tile_instances_cpu.py checks the table against the sources and against a Python restatement of the rules;
tests/test_gpu_tile_instances.py runs every case: tag, fp64 reference, and a slice re-run through a small launch.
profiles/tile_instances.md has the measured errors.

The rules, for reference (cdiv = ceiling division):
  choose_tile(m, n): WN = 1 for n <= 64 else 2; MI = 2 iff cdiv(m, (4 / WN) * 64) * cdiv(n, WN * 64) >= 512
  wide(m, n, K, batch): n >= 256, K % 32 == 0, small = cdiv(m, 128) * cdiv(n, 256) * batch >= 192;
      256 x 256 (<4,2,4>) iff big = cdiv(m, 256) * cdiv(n, 256) * batch >= 224 and 100 * cdiv(big, 256) <= 55 * cdiv(small, 256),
      128 x 256 (<2,2,4>) otherwise
"""

CT = "choose_tile(m, n)"
FAMILIES = {
    # exact-fp32 linear_kernel<MI,WN,BK>: BK = 16 with MI = 2, 32 otherwise; bgemm_nt chooses with m * batch rows
    "linear_f32": {"linear_f32<1,1,32>": CT, "linear_f32<1,2,32>": CT, "linear_f32<2,1,16>": CT, "linear_f32<2,2,16>": CT},
    # single-product fp16 linear_f16_kernel<MI,WN>: WN = 1 always runs MI = 1 (the 256-row instantiation spills)
    "linear_f16": {"linear_f16<1,1>": CT + ", any m for n <= 64", "linear_f16<1,2>": CT, "linear_f16<2,2>": CT},
    # split-fp16, fp32 A: narrow linear_x3_kernel<MI,WN> when the wide rule says no
    "linear_x3": {"linear_x3<1,1>": "not wide; " + CT, "linear_x3<1,2>": "not wide; " + CT, "linear_x3<2,1>": "not wide; " + CT,
                  "linear_x3<2,2>": "not wide; " + CT},
    # ... with the LayerNorm + GELU operand transform (second GEMM of an MLP tail; n > 64 is required, so WN = 2)
    "linear_x3/lngelu": {"linear_x3<1,2,lngelu>": "not wide; " + CT, "linear_x3<2,2,lngelu>": "not wide; " + CT},
    # split-fp16, A as planes: linear_x3p_kernel<MI,WN>; the batched form chooses with one batch element's m
    "linear_x3p": {"linear_x3p<1,1>": "not wide; " + CT, "linear_x3p<1,2>": "not wide; " + CT, "linear_x3p<2,1>": "not wide; " + CT,
                   "linear_x3p<2,2>": "not wide; " + CT},
    # wide tiles linear_x3w_kernel<MI,WM,WN,...>
    "linear_x3w": {"linear_x3w<2,2,4>": "wide, 128 x 256", "linear_x3w<4,2,4>": "wide, 256 x 256"},
    "linear_x3w/planes": {"linear_x3w<2,2,4,planes>": "wide, 128 x 256", "linear_x3w<4,2,4,planes>": "wide, 256 x 256"},
    "linear_x3w/lngelu": {"linear_x3w<2,2,4,lngelu>": "wide, 128 x 256", "linear_x3w<4,2,4,lngelu>": "wide, 256 x 256"},
    # exact-fp32 conv_kernel<false,MI,WN,BK>: BK = 16 for WN = 1, else 32; m = batch * ho * wo
    "conv_f32": {"conv_f32<1,1,16>": CT, "conv_f32<1,2,32>": CT, "conv_f32<2,1,16>": CT, "conv_f32<2,2,32>": CT},
    # the stem's 4-channel input: conv_kernel<true,2,WN,16>, MI = 2 whatever the grid
    "conv_f32_cin4": {"conv_f32_cin4<2,1,16>": "cin == 4, cout <= 64", "conv_f32_cin4<2,2,16>": "cin == 4, cout > 64"},
    "conv_f16": {"conv_f16<1,1>": CT, "conv_f16<1,2>": CT, "conv_f16<2,1>": CT, "conv_f16<2,2>": CT},
    # split-fp16 convolution: halo (3x3 / stride 1, cout == 128 or >= 256, >= 224 spatial tiles of 8 x 32 times column tiles),
    # then the wide tile (cout >= 256, cdiv(m, 256) * cdiv(cout, 256) >= 224), then conv_x3_kernel<MI,WN>
    "conv_x3h": {"conv_x3h<2>": "3x3 s1, cout == 128, batch * cdiv(wo, 32) * cdiv(ho, 8) >= 224",
                 "conv_x3h<4>": "3x3 s1, cout >= 256, batch * cdiv(wo, 32) * cdiv(ho, 8) * cdiv(cout, 256) >= 224"},
    "conv_x3w": {"conv_x3w<4,2,4>": "not halo, cout >= 256, cdiv(m, 256) * cdiv(cout, 256) >= 224"},
    "conv_x3": {"conv_x3<1,1>": "not halo, not wide; " + CT, "conv_x3<1,2>": "not halo, not wide; " + CT,
                "conv_x3<2,1>": "not halo, not wide; " + CT, "conv_x3<2,2>": "not halo, not wide; " + CT},
    # attention_x3_pipe_kernel<PSPLIT,false,MODE,NWV,PHASES>.  ps / p1: probabilities as two fp16 parts (always below 1024 keys;
    # pram_attention_x3_set_p_split from there on).  mode 0: one key chunk per sequence (n_max < 1024 or n_max <= chunk keys),
    # eight waves in the phases form iff batch * heads * cdiv(m_max, 256) >= 256, else four waves interleaved.  Several chunks:
    # mode 1 (fused: no workspace, or split groups < 2), mode 2 (split); phases iff grid.x * grid.y >= 512 and a workgroup walks
    # >= 32 key tiles.
    "attention_x3_pipe": {f"attention_x3_pipe<{ps},mode{mode},w{w},{form}>": rule
                          for ps in ("ps", "p1")
                          for mode, w, form, rule in ((0, 8, "phases", "one chunk, batch * heads * cdiv(m_max, 256) >= 256"),
                                                      (0, 4, "interleaved", "one chunk, fewer 256-row units"),
                                                      (1, 4, "phases", "chunks, fused, grid >= 512 and >= 32 tiles"),
                                                      (1, 4, "interleaved", "chunks, fused, smaller"),
                                                      (2, 4, "phases", "chunks, split, grid.x * groups >= 512 and >= 32 tiles per group"),
                                                      (2, 4, "interleaved", "chunks, split, smaller"))},
    # attention_x3_pipe_kernel<false,true,0,NWV>: the single-product form
    "attention_h16t": {"attention_h16t<8>": "batch * heads * cdiv(m_max, 256) >= 256", "attention_h16t<4>": "fewer"},
}

# absolute bars against fp64, each the one the existing test of that path uses
BARS = {
    "linear_x3": (4e-6, "tests/test_gpu_x3.py:47"),                    # also the planes GEMM (tests/test_gpu_x3.py:278)
    "linear_f32": (2e-5, "tests/test_gpu_kernels.py:40"),
    "linear_f16": (2e-5, "tests/test_gpu_kernels.py:65"),              # against fp64 on the fp16-rounded operands
    "planes_rel": (2.0 ** -21, "tests/test_gpu_x3.py:94"),             # hi + lo against the fp32 result, |v| >= 2^-7 (2^-29 absolute below)
    "mlp_tail": (2e-5, "tests/test_gpu_guard_chunks_mlp.py:514"),
    "conv_x3": (1e-5, "tests/test_gpu_x3.py:328"),
    "conv_f32": (2e-5, "tests/test_gpu_kernels.py:386"),
    "conv_f16": (2e-5, "tests/test_gpu_kernels.py:82"),                # against fp64 on the fp16-rounded operands
    "attention_x3_short": (3e-6, "tests/test_gpu_x3.py:145"),          # n_max < 1024
    "attention_x3_ps": (2e-6, "tests/test_gpu_guard_chunks_mlp.py:386"),      # from 1024 keys on, probabilities as two parts
    "attention_x3_p1": (2e-4, "tests/test_gpu_guard_chunks_mlp.py:386"),      # ... as one fp16
    "attention_h16t": (5e-4, "tests/test_gpu_x3.py:307"),              # against fp64 on the fp16 operands
}

CASES = []


def _add(entry, tag, bar, **kw):
    CASES.append(dict(entry=entry, tag=tag, bar=bar, **kw))


# ------------------------------------------------------------------------------------------------ linear, split-fp16, fp32 A
# first shape of every instantiation: every epilogue; the others: bias + residual + alpha.  The smallest m of a rule + 5 leaves a last
# tile of 6 rows (its first 32-row accumulator block only); + 100 puts rows of the second block into the ragged tile as well
EPILOGUES = ("bias_res_alpha", "x2", "rotary", "split_also", "lens")
X3_SHAPES = {
    "linear_x3<1,1>": [(300, 64)],
    "linear_x3<1,2>": [(300, 136)],
    "linear_x3<2,1>": [(130822, 64), (130822, 40), (130917, 64)],          # cdiv(m, 256) = 512
    "linear_x3<2,2>": [(32646, 136), (65414, 128), (32741, 136)],          # cdiv(m, 128) * 2 = 512; cdiv(m, 128) = 512
    "linear_x3w<2,2,4>": [(24449, 256), (12161, 264), (24549, 256)],       # small = 192, big = 96
    "linear_x3w<4,2,4>": [(57094, 256), (28422, 264), (57189, 256)],       # big = 224, small = 447 / 446: one round against two
}
for _tag, _shapes in X3_SHAPES.items():
    for _i, (_m, _n) in enumerate(_shapes):
        for _epi in (EPILOGUES if _i == 0 else ("bias_res_alpha",)):
            _add("linear", _tag, "linear_x3", prec="x3", m=_m, n=_n, k=64, epi=_epi)

# ------------------------------------------------------------------------------------------------ linear, exact fp32 and fp16
for _tag, _m, _n in (("linear_f32<1,1,32>", 300, 40), ("linear_f32<1,2,32>", 300, 136), ("linear_f32<2,1,16>", 130822, 64),
                     ("linear_f32<2,1,16>", 130822, 40), ("linear_f32<2,1,16>", 130917, 64), ("linear_f32<2,2,16>", 32646, 136), ("linear_f32<2,2,16>", 65414, 128)):
    _add("linear", _tag, "linear_f32", prec="f32", m=_m, n=_n, k=32, epi="bias_res_alpha")
for _tag, _m, _n in (("linear_f16<1,1>", 300, 40), ("linear_f16<1,1>", 130822, 64), ("linear_f16<1,2>", 300, 136),
                     ("linear_f16<2,2>", 32646, 136), ("linear_f16<2,2>", 65414, 128), ("linear_f16<2,2>", 32741, 136)):
    _add("linear", _tag, "linear_f16", prec="f16", m=_m, n=_n, k=64, epi="bias_res_alpha")

# ------------------------------------------------------------------------------------------------ linear_planes (A as planes)
for _tag, _m, _n in (("linear_x3p<1,1>", 300, 40), ("linear_x3p<1,2>", 300, 136), ("linear_x3p<2,1>", 130822, 64), ("linear_x3p<2,1>", 130917, 64),
                     ("linear_x3p<2,2>", 32646, 136), ("linear_x3w<2,2,4,planes>", 24449, 256), ("linear_x3w<4,2,4,planes>", 57094, 256)):
    _add("linear_planes", _tag, "linear_x3", m=_m, n=_n, k=64, epi="bias_res_alpha")
    if _m > 300:
        _add("linear_planes", _tag, "linear_x3", m=_m, n=_n, k=64, epi="x2")

# ------------------------------------------------------------------------------------------------ q | k | v projection
# n = q columns + heads * 64 value columns; sequences of 64 tokens, ragged lengths, rotary on the first 64 columns
for _tag, _m, _n, _heads in (("linear_x3<1,2>", 320, 128, 1), ("linear_x3<2,2>", 65536, 128, 1),
                             ("linear_x3w<2,2,4>", 24512, 256, 2), ("linear_x3w<4,2,4>", 57152, 256, 2)):
    _add("linear_qkv_planes", _tag, "linear_x3", m=_m, n=_n, k=64, heads=_heads, t_seq=64)

# ------------------------------------------------------------------------------------------------ MLP tail: both GEMMs
# tag_first: the ssq writer (k -> hid), tag: the LayerNorm + GELU consumer (hid -> n)
for _first, _tag, _m, _hid, _n in (("linear_x3<1,2>", "linear_x3<1,2,lngelu>", 300, 128, 136),
                                   ("linear_x3<2,1>", "linear_x3<2,2,lngelu>", 130822, 64, 128),
                                   ("linear_x3<2,2>", "linear_x3<2,2,lngelu>", 65414, 128, 136),
                                   ("linear_x3w<2,2,4>", "linear_x3w<2,2,4,lngelu>", 24449, 256, 256),
                                   ("linear_x3w<4,2,4>", "linear_x3w<4,2,4,lngelu>", 57094, 256, 256)):
    _add("mlp_tail", _tag, "mlp_tail", tag_first=_first, m=_m, k=64, hid=_hid, n=_n)

# ------------------------------------------------------------------------------------------------ batched A . B^T
# exact fp32: tiles are cut from batch * m rows.  m = 128: a <2,2,16> tile is exactly one batch element; m = 130: ragged last tile
for _tag, _b, _m in (("linear_f32<1,2,32>", 3, 130), ("linear_f32<2,2,16>", 512, 128), ("linear_f32<2,2,16>", 512, 130)):
    _add("bgemm_nt", _tag, "linear_f32", batch=_b, m=_m, n=128, k=32)
# planes: 128 x 256 with 100 real rows per tile; 256 x 256 with 130 real rows in the first tile of every batch element
for _tag, _b, _m, _n in (("linear_x3p<1,2>", 3, 100, 136), ("linear_x3w<2,2,4,planes>", 192, 100, 256), ("linear_x3w<4,2,4,planes>", 224, 130, 256)):
    _add("bgemm_nt_planes", _tag, "linear_x3", batch=_b, m=_m, n=_n, k=64)

# ------------------------------------------------------------------------------------------------ convolutions
# every shape in the plain form and with bias + BN scale / shift + residual + ReLU
CONV_SHAPES = [
    # tag suffix, (B, H, W), cout, ks, stride
    ("<1,1>", (1, 24, 33), 40, 3, 1),
    ("<1,2>", (1, 24, 33), 136, 1, 1),
    ("<2,1>", (2, 256, 256), 64, 3, 1),            # m = 131072 >= 130817
    ("<2,1>", (2, 256, 256), 40, 3, 1),
    ("<2,1>", (2, 256, 256), 64, 1, 1),
    ("<2,1>", (2, 512, 512), 64, 3, 2),
    ("<2,2>", (1, 256, 256), 128, 1, 1),           # m = 65536 >= 65409; cout 128 off the halo path
    ("<2,2>", (1, 512, 512), 128, 3, 2),
]
for _sfx, _bhw, _cout, _ks, _st in CONV_SHAPES:
    for _form in ("plain", "full"):
        _add("conv", "conv_x3" + _sfx, "conv_x3", prec="x3", bhw=_bhw, cin=32, cout=_cout, ks=_ks, stride=_st, form=_form)
        if (_cout, _ks, _st) in ((40, 3, 1), (136, 1, 1), (64, 3, 1), (128, 1, 1), (128, 3, 2)):      # the same m and n on the other two paths
            _bk = ",16>" if _cout <= 64 else ",32>"
            _add("conv", "conv_f32" + _sfx[:-1] + _bk, "conv_f32", prec="f32", bhw=_bhw, cin=32, cout=_cout, ks=_ks, stride=_st, form=_form)
            _add("conv", "conv_f16" + _sfx, "conv_f16", prec="f16", bhw=_bhw, cin=64, cout=_cout, ks=_ks, stride=_st, form=_form)
for _form in ("plain", "full"):
    # halo: 3 x cdiv(160, 32) x cdiv(120, 8) = 225 spatial tiles
    _add("conv", "conv_x3h<2>", "conv_x3", prec="x3", bhw=(3, 120, 160), cin=32, cout=128, ks=3, stride=1, form=_form)
    _add("conv", "conv_x3h<4>", "conv_x3", prec="x3", bhw=(3, 120, 160), cin=32, cout=256, ks=3, stride=1, form=_form)
    # wide tile off the halo path: 1x1, cdiv(241 * 240, 256) = 226; cdiv(170 * 171, 256) * 2 = 228; stride 2: cdiv(240 * 241, 256) = 226
    _add("conv", "conv_x3w<4,2,4>", "conv_x3", prec="x3", bhw=(1, 241, 240), cin=32, cout=256, ks=1, stride=1, form=_form)
    _add("conv", "conv_x3w<4,2,4>", "conv_x3", prec="x3", bhw=(1, 170, 171), cin=32, cout=264, ks=1, stride=1, form=_form)
    _add("conv", "conv_x3w<4,2,4>", "conv_x3", prec="x3", bhw=(1, 480, 481), cin=32, cout=256, ks=3, stride=2, form=_form)
    # the stem's 4-channel input
    _add("conv", "conv_f32_cin4<2,1,16>", "conv_f32", prec="f32", bhw=(1, 48, 65), cin=4, cout=64, ks=3, stride=1, form=_form)
    _add("conv", "conv_f32_cin4<2,2,16>", "conv_f32", prec="f32", bhw=(1, 48, 65), cin=4, cout=96, ks=3, stride=1, form=_form)

# ------------------------------------------------------------------------------------------------ split-fp16 attention
# ragged q_lens / k_lens everywhere; chunk = pram_attention_x3_set_chunk_keys, split = a workspace is handed over,
# target = pram_attention_x3_set_split_target
_add("attention_x3", "attention_x3_pipe<ps,mode0,w8,phases>", "attention_x3_short", batch=64, m=130, n=65, kv_shift=0)
_add("attention_x3", "attention_x3_pipe<ps,mode0,w8,phases>", "attention_x3_short", batch=64, m=130, n=65, kv_shift=32)
_add("attention_x3", "attention_x3_pipe<ps,mode0,w4,interleaved>", "attention_x3_short", batch=3, m=130, n=65, kv_shift=0)
for _ps in (1, 0):
    _p, _bar = ("ps", "attention_x3_ps") if _ps else ("p1", "attention_x3_p1")
    _kw = dict(p_split=_ps, kv_shift=0)
    _add("attention_x3", f"attention_x3_pipe<{_p},mode0,w8,phases>", _bar, batch=16, m=1024, n=1100, **_kw)
    _add("attention_x3", f"attention_x3_pipe<{_p},mode0,w4,interleaved>", _bar, batch=2, m=300, n=1100, **_kw)
    _add("attention_x3", f"attention_x3_pipe<{_p},mode1,w4,interleaved>", _bar, batch=2, m=300, n=1100, chunk=512, split=False, **_kw)
    _add("attention_x3", f"attention_x3_pipe<{_p},mode1,w4,phases>", _bar, batch=8, m=2048, n=2048, chunk=512, split=False, **_kw)
    _add("attention_x3", f"attention_x3_pipe<{_p},mode2,w4,interleaved>", _bar, batch=2, m=300, n=1100, chunk=512, split=True, **_kw)
    _add("attention_x3", f"attention_x3_pipe<{_p},mode2,w4,phases>", _bar, batch=4, m=2048, n=4096, chunk=512, split=True, target=512, **_kw)
_add("attention_h16t", "attention_h16t<8>", "attention_h16t", batch=64, m=300, n=517, kv_shift=0)
_add("attention_h16t", "attention_h16t<8>", "attention_h16t", batch=64, m=300, n=517, kv_shift=32)
_add("attention_h16t", "attention_h16t<4>", "attention_h16t", batch=3, m=300, n=517, kv_shift=0)


def case_id(c):
    skip = ("entry", "tag", "bar", "tag_first")
    return c["entry"] + "-" + c["tag"] + "-" + "-".join(
        f"{k}{'x'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in c.items() if k not in skip)


def all_tags():
    return {t for fam in FAMILIES.values() for t in fam}
