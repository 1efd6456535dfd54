"""GPU (MI355X): the split-fp16 ("x3") path at every activation scale it can run at (include/pram_hip.h, "activation scale";
DESIGN §4.8).  The planes carry value * s; the range guard walks s = 16 -> 1 -> ... -> ops.ACT_SCALE_MIN and the C ABI accepts
any power of two down to 2^-12.

1. exact rescaling: scaling the inputs by 2^k while lowering s by 2^-k leaves the planes bit-identical, and every fp32 epilogue
   step is then an exact power-of-two rescale — so every entry point must give 2^k times its bits.  A launcher that stages under
   one scale and undoes another, or a kernel that applies 1/s on the wrong side, fails here at once.
   Not exactly homogeneous, so covered by section 2 only: the LayerNorm + GELU staging (eps, GELU) and the l2norm epilogue (eps).
2. accuracy against fp64 at every scale, against the error model of DESIGN §4.8.
3. the range edge (|s x| = 65504 fits, 65520 does not) at every scale and at every plane-writing site.
4. the models at every scale the guard can reach (golden vectors, the usual bars).
5. the guard's real descent inside a pipeline, against the same run on the exact-fp32 kernels."""
import math

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from pram_amd import ops, weights as W
from tests import helpers as H

pytestmark = pytest.mark.gpu

# the guard's ladder: 16, 1, 1/16, ... down to ACT_SCALE_MIN (derived, so the tests follow the constant)
LADDER = [ops.ACT_SCALE_DEFAULT * 16.0 ** -i for i in range(8) if ops.ACT_SCALE_DEFAULT * 16.0 ** -i >= ops.ACT_SCALE_MIN]
ABI_MIN = 2.0 ** -12                                   # the lowest scale the C ABI accepts
SCALES = sorted(set(LADDER) | {ABI_MIN}, reverse=True)
KS = (4, 8, 12, 16)                                     # 2^k: s = 16 * 2^-k reaches 2^-12

# Error model of one split product: x s = hi + lo loses at most 2^-22 |x| (hi and lo both normal fp16) or 2^-25 / s
# absolute (lo, or hi itself, subnormal); the same for the weight (its own scale); the dropped lo . lo term is <= 2^-22 |a w|.
# Three 2^-22 terms = 1.5 * 2^-21; the fp32 accumulation of the MFMAs and the epilogue's rounding add at most another 2^-22
# relative to sum |a w| in these sizes: C = 2.
C = 2.0


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(seed, shape, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * std


def _logu(seed, shape, s, lo=-20.0, hi=11.0):
    """random signs, log-uniform magnitudes over [2^lo, 2^hi], clipped to 65504 / s (the largest value the planes carry)"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).clamp(max=65504.0 / s)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def _planes(x, s):
    """the split format itself (round to nearest, as the kernels' conversions): x s = hi + lo"""
    xs = x.float() * s
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return hi.contiguous(), lo.contiguous()


def _val(pl, s):
    return (pl[0].double() + pl[1].double()) / s


def _clear(dev):
    ops.x3_range_exceeded(dev)


def _no_flag(dev):
    assert not ops.x3_range_exceeded(dev), "range flag raised on in-range data"


# ================================================================================================ 1. exact power-of-two rescaling
def _rescaled(dev, fn, ks=KS):
    """fn(m, s) -> tuple of tensors computed from inputs multiplied by m under activation scale s.  Asserts, for every k, that
    fn(2^k, 16 * 2^-k) equals fn(1, 16) rescaled as fn says (fn returns (tensor, power) pairs: the tensor must scale by 2^(k power))."""
    _clear(dev)
    with ops.act_scale_scope(16.0):
        base = fn(1.0, 16.0)
    _no_flag(dev)
    for k in ks:
        m, s = 2.0 ** k, 16.0 * 2.0 ** -k
        with ops.act_scale_scope(s):
            got = fn(m, s)
        _no_flag(dev)
        for i, ((b, p), (g, _)) in enumerate(zip(base, got)):
            if b.dtype == torch.float16:          # planes: bit-identical
                assert torch.equal(g, b), (k, i)
            else:
                assert torch.equal(g, b * (2.0 ** (k * p))), (k, i, float((g - b * 2.0 ** (k * p)).abs().max()))
    assert ops.current_act_scale() == 16.0


def test_linear_rescales_exactly(dev):
    """bias, residual, alpha, rotary, a concatenated second segment, the ragged form; fp32 output and planes"""
    m, k0, k1, n = 300, 128, 64, 384
    x, x2 = _rand(1, (m, k0)).to(dev), _rand(2, (m, k1)).to(dev)
    w = _rand(3, (n, k0 + k1), (k0 + k1) ** -0.5).to(dev)
    b, res = _rand(4, (n,), 0.3).to(dev), _rand(5, (m, n)).to(dev)
    ang = W.uniform(3, "as1/a", (m, 32), -3.0, 3.0)
    rot = (torch.cos(ang).to(dev), torch.sin(ang).to(dev), 256)
    lens = torch.tensor([150, 61], dtype=torch.int32, device=dev)

    w0 = w[:, :k0].contiguous()

    def f(mul, s):
        y = ops.linear(x * mul, w, b * mul, x2=x2 * mul, residual=res * mul, alpha=0.75, rotary=rot, precision="x3")
        y2, pl = ops.linear(x * mul, w, b * mul, x2=x2 * mul, alpha=1.5, split_out="also", precision="x3")
        out = torch.zeros(m, n, device=dev)
        ops.linear(x * mul, w0, b * mul, residual=res * mul, lens=lens, t_pad=150, out=out, precision="x3")
        valid = torch.cat([out[:150], out[150:211]])
        return [(y, 1), (y2, 1), (pl[0], 0), (pl[1], 0), (valid, 1)]
    _rescaled(dev, f)


def test_linear_planes_and_qkv_planes_rescale_exactly(dev):
    """planes in -> planes out (linear_planes); the q / k planes and the transposed value planes of the qkv projection"""
    m, k, n = 320, 256, 192
    x = _rand(11, (m, k)).to(dev)
    w1 = _rand(12, (256, k), k ** -0.5).to(dev)
    b1 = _rand(13, (256,), 0.2).to(dev)
    w2 = _rand(14, (n, 256), 256 ** -0.5).to(dev)
    b2, res = _rand(15, (n,), 0.2).to(dev), _rand(16, (m, n)).to(dev)
    wq, bq = _rand(17, (768, k), k ** -0.5).to(dev), _rand(18, (768,), 0.2).to(dev)
    ang = W.uniform(3, "as2/a", (2 * 192, 32), -3.0, 3.0)
    rot = (torch.cos(ang).to(dev), torch.sin(ang).to(dev), 512)
    lens = torch.tensor([192, 131], dtype=torch.int32, device=dev)
    xq = _rand(19, (2 * 192, k)).to(dev)

    def f(mul, s):
        _, pl = ops.linear(x * mul, w1, b1 * mul, split_out="only", precision="x3")
        y, pl2 = ops.linear_planes(pl, w2, b2 * mul, residual=res * mul, alpha=0.5, out="both")
        qk, vt = ops.linear_qkv_planes(xq * mul, wq, bq * mul, 4, 192, rotary=rot, lens=lens)
        rows = lambda t: torch.cat([t[:192], t[192:192 + 131]])      # q / k rows beyond lens are never written
        return [(pl[0], 0), (pl[1], 0), (y, 1), (pl2[0], 0), (pl2[1], 0), (rows(qk[0]), 0), (rows(qk[1]), 0), (vt[0], 0), (vt[1], 0)]
    _rescaled(dev, f)


def test_mlp_tail_first_gemm_and_bgemm_rescale_exactly(dev):
    """pram_linear_x3_ssq_f32 as ops.mlp_tail calls it (output x 2^k, row sums of squares x 2^2k); bgemm_nt_planes (x 2^2k)"""
    L = ops._lib.load()
    m, k, hid = 300, 256, 512
    x = _rand(21, (m, k)).to(dev)
    w0c, b0c = [t.to(dev) for t in ops.center_linear(_rand(22, (hid, k), k ** -0.5), _rand(23, (hid,), 0.3) + 0.7)]
    lens = torch.tensor([150, 97], dtype=torch.int32, device=dev)
    B, M, N = 2, 150, 140
    xa, xb = _rand(24, (B * M, 256)).to(dev), _rand(25, (B * N, 256)).to(dev)
    wa = _rand(26, (128, 256), 256 ** -0.5).to(dev)

    def f(mul, s):
        parts = int(L.pram_linear_x3_ssq_parts(m, hid, k))
        h = torch.zeros(m, hid, device=dev)
        ssq = torch.zeros(parts, m, device=dev)
        wh, wl, ws = ops.split_weight(w0c)
        xm = (x * mul).contiguous()
        bm = (b0c * mul).contiguous()
        ops._lib.check(L.pram_linear_x3_ssq_f32(xm.data_ptr(), k, k, None, 0, 0, wh.data_ptr(), wl.data_ptr(), ws, bm.data_ptr(),
                                                h.data_ptr(), hid, ssq.data_ptr(), m, hid, lens.data_ptr(), 150, ops._st()), "ssq")
        valid = torch.cat([h[:150], h[150:247]])
        vs = torch.cat([ssq[:, :150], ssq[:, 150:247]], 1)
        _, pa = ops.linear(xa * mul, wa, None, split_out="only", precision="x3")
        _, pb = ops.linear(xb * mul, wa, None, split_out="only", precision="x3")
        c = ops.bgemm_nt_planes(pa, pb, B, M, N, alpha=0.5)
        return [(valid, 1), (vs, 2), (c, 2)]
    _rescaled(dev, f)


def test_convolutions_rescale_exactly(dev):
    """conv2d_nhwc (bias, BatchNorm scale / shift, residual, ReLU; 1x1, 3x3, stride 2), conv2d_nhwc_planes,
    conv3x3_grouped_planes, the fused sfd2_conv1"""
    B, Hh, Ww, cin, cout = 2, 19, 23, 64, 96
    x = _rand(31, (B, Hh, Ww, cin)).to(dev)
    w3 = _rand(32, (cout, 3, 3, cin), (9 * cin) ** -0.5).to(dev)
    w1 = _rand(33, (128, 1, 1, cin), cin ** -0.5).to(dev)
    bias, sc, sh = _rand(34, (cout,), 0.1).to(dev), (1.0 + _rand(35, (cout,), 0.1)).to(dev), _rand(36, (cout,), 0.1).to(dev)
    res = _rand(37, (B, Hh, Ww, cout)).to(dev)
    sc1, sh1 = (1.0 + _rand(38, (128,), 0.1)).to(dev), _rand(39, (128,), 0.1).to(dev)
    wg = _rand(40, (128, 3, 3, 8), (72.0) ** -0.5).to(dev)
    scg, shg = (1.0 + _rand(41, (128,), 0.1)).to(dev), _rand(42, (128,), 0.1).to(dev)
    img = _rand(43, (2, 3, 37, 45)).to(dev)
    wa, wb = _rand(44, (64, 3, 3, 4), 0.2).to(dev), _rand(45, (64, 3, 3, 64), (576.0) ** -0.5).to(dev)
    wa[..., 3] = 0.0
    ba, sa, ta = _rand(46, (64,), 0.1).to(dev), (1.0 + _rand(47, (64,), 0.1)).to(dev), _rand(48, (64,), 0.1).to(dev)
    bb, sb, tb = _rand(49, (64,), 0.1).to(dev), (1.0 + _rand(50, (64,), 0.1)).to(dev), _rand(51, (64,), 0.1).to(dev)

    def f(mul, s):
        y = ops.conv2d_nhwc(x * mul, w3, bias * mul, sc, sh * mul, residual=res * mul, ks=3, relu=True, precision="x3")
        y2 = ops.conv2d_nhwc(x * mul, w3, bias * mul, ks=3, stride=2, precision="x3")
        hi, lo = ops.conv2d_nhwc_planes(x * mul, w1, None, sc1, sh1 * mul, ks=1, relu=True)
        g = ops.conv3x3_grouped_planes(hi, lo, wg, scg, shg * mul, 16, True)
        c1 = ops.sfd2_conv1(img * mul, wa, ba * mul, sa, ta * mul, wb, bb * mul, sb, tb * mul)
        return [(y, 1), (y2, 1), (hi, 0), (lo, 0), (g, 1), (c1, 1)]
    _rescaled(dev, f)


@pytest.fixture
def attn_modes():
    """restores the process-wide attention knobs (chunk keys, split target, P split) after the test"""
    L = ops._lib.load()
    ck, ps, saved = L.pram_attention_x3_set_chunk_keys(0), L.pram_attention_x3_set_p_split(-1), ops.attention_split
    yield L
    L.pram_attention_x3_set_chunk_keys(ck)
    L.pram_attention_x3_set_p_split(ps)
    L.pram_attention_x3_set_split_target(-1)
    ops.attention_split = saved


@pytest.mark.parametrize("p_split", [1, 0])
def test_attention_rescales_exactly(dev, attn_modes, p_split):
    """attention_x3 fused and split (workspace), ragged lens, probabilities in two parts and in one, the cross form (kv_shift),
    attention_colmean_x3: q, k, v x 2^k and the soft-max scale x 2^-2k give the output x 2^k, the same log-sum-exps and the
    same column means"""
    L = attn_modes
    L.pram_attention_x3_set_p_split(p_split)
    S, T, T1 = 2, 192, 1024
    x = _rand(61, (S * T, 256)).to(dev)
    x1 = _rand(62, (T1, 256)).to(dev)
    wq, bq = _rand(63, (768, 256), 256 ** -0.5).to(dev), _rand(64, (768,), 0.2).to(dev)
    wc, bc = _rand(65, (512, 256), 256 ** -0.5).to(dev), _rand(66, (512,), 0.2).to(dev)
    lens = torch.tensor([192, 117], dtype=torch.int32, device=dev)
    l1 = torch.tensor([T1 - 37], dtype=torch.int32, device=dev)

    def f(mul, s):
        sc = 0.125 / (mul * mul)
        out = []
        pl, vt = ops.linear_qkv_planes(x * mul, wq, bq * mul, 4, T, lens=lens)
        q3, k3 = (pl[0][:, :256], pl[1][:, :256]), (pl[0][:, 256:512], pl[1][:, 256:512])
        for split in (False, True):
            ops.attention_split = split
            o, lse = ops.attention_x3(q3, k3, vt, S, 4, T, T, sc, lens, lens, want_lse=True)
            out += [(torch.cat([o[:192], o[192:192 + 117]]), 1), (torch.cat([lse[0], lse[1, :, :117]], 1), 0)]
        out.append((ops.attention_colmean_x3(q3, k3, lse, S, 4, T, T, sc, lens, lens), 0))
        # cross form: sequence 0 attends to sequence 1 and vice versa (the matcher's cross layers)
        plc, vtc = ops.linear_qkv_planes(x * mul, wc, bc * mul, 4, T, lens=lens)
        qk = (plc[0][:, :256], plc[1][:, :256])
        o, lse = ops.attention_x3(qk, qk, vtc, S, 4, T, T, sc, lens, lens, want_lse=True, kv_shift=1)
        out += [(torch.cat([o[:192], o[192:192 + 117]]), 1), (ops.attention_colmean_x3(qk, qk, lse, S, 4, T, T, sc, lens, lens, kv_shift=1), 0)]
        # one long sequence with 512-key chunks: the split mode runs the chunks as a grid dimension
        L.pram_attention_x3_set_chunk_keys(512)
        assert L.pram_attention_x3_is_split(1, 4, T1, T1) > 1
        pl1, vt1 = ops.linear_qkv_planes(x1 * mul, wq, bq * mul, 4, T1, lens=l1)
        q1, k1 = (pl1[0][:, :256], pl1[1][:, :256]), (pl1[0][:, 256:512], pl1[1][:, 256:512])
        for split in (False, True):
            ops.attention_split = split
            o = ops.attention_x3(q1, k1, vt1, 1, 4, T1, T1, sc, l1, l1)
            out.append((o[:T1 - 37], 1))
        L.pram_attention_x3_set_chunk_keys(4096)
        ops.attention_split = True
        return out
    _rescaled(dev, f)


# ================================================================================================ 2. accuracy against fp64
def _gemm_bound(a, w, s, ws, ref):
    """per-element bound of a split-fp16 product a @ w.T (a at scale s, w at scale ws), fp64 operands"""
    f = C * (2.0 ** -21 * (a.abs() @ w.abs().t()) + 2.0 ** -25 / s * w.abs().sum(1)[None] + 2.0 ** -25 / ws * a.abs().sum(1)[:, None])
    return f + 2.0 ** -23 * ref.abs()


def _emulated(a, w, s, ws, lo_a=True):
    """the three products in fp64 on the split operands (lo_a=False: the activations' lo plane dropped)"""
    ah, al = _planes(a, s)
    wh, wl = _planes(w, ws)
    ah, al, wh, wl = ah.double() / s, (al.double() / s if lo_a else 0 * al.double()), wh.double() / ws, wl.double() / ws
    return ah @ wh.t() + ah @ wl.t() + al @ wh.t()


def _worst(name, s, err, bound, log):
    r = float((err / bound).max())
    log.append(f"{name} s=2^{int(math.log2(s))}: max|err| {float(err.max()):.2e}, max err/bound {r:.3f}")
    assert r <= 1.0, log[-1]


@pytest.mark.parametrize("s", SCALES)
def test_linear_and_bgemm_accuracy_against_fp64(dev, s):
    """linear (staging split), linear_planes (planes in), bgemm_nt_planes (both operands planes) on inputs spanning every
    regime of the split (both parts normal, lo subnormal, hi subnormal) against fp64 and the per-element error model; and the
    model is tight: the same products with the lo plane dropped violate it."""
    log = []
    m, k, n = 200, 256, 192
    a = _logu(71, (m, k), s).to(dev)
    w = _rand(72, (n, k), k ** -0.5).to(dev)
    ws = ops.split_weight(w)[2]
    ref = a.double() @ w.double().t()
    bound = _gemm_bound(a.double(), w.double(), s, ws, ref)
    _clear(dev)
    with ops.act_scale_scope(s):
        y = ops.linear(a, w, precision="x3")
        yp = ops.linear_planes(_planes(a, s), w)
    _no_flag(dev)
    _worst("linear", s, (y.double() - ref).abs(), bound, log)
    _worst("linear_planes", s, (yp.double() - ref).abs(), bound, log)
    # the bound bites: dropping lo (error ~2^-12 s x relative) breaks it; the exact emulation of the three products keeps it
    assert bool(((_emulated(a, w, s, ws, lo_a=False) - ref).abs() > bound).any())
    assert bool(((_emulated(a, w, s, ws) - ref).abs() <= bound).all())
    # bgemm: both operands are planes at s
    B, M, N = 2, 96, 80
    pa, pb = _logu(73, (B * M, k), s).to(dev), _logu(74, (B * N, k), s, hi=2.0).to(dev)
    with ops.act_scale_scope(s):
        c = ops.bgemm_nt_planes(_planes(pa, s), _planes(pb, s), B, M, N)
    for z in range(B):
        A, Bm = pa[z * M:(z + 1) * M].double(), pb[z * N:(z + 1) * N].double()
        r = A @ Bm.t()
        _worst("bgemm", s, (c[z].double() - r).abs(), _gemm_bound(A, Bm, s, s, r), log)
    print("; ".join(log))


@pytest.mark.parametrize("s", SCALES)
def test_mlp_tail_conv_l2norm_and_conv1_accuracy_against_fp64(dev, s):
    """the LayerNorm + GELU staging (ops.mlp_tail), a convolution with the fused l2norm epilogue, the fused sfd2_conv1"""
    log = []
    # ---- mlp tail: h = x w0c^T + b0c (fp32 + row sums of squares), out = GELU(LN(h)) w3^T + b3 + residual
    m, k, hid, n = 200, 256, 256, 192
    x = _logu(81, (m, k), s).to(dev)
    w0, b0 = _rand(82, (hid, k), k ** -0.5), _rand(83, (hid,), 0.3) + 0.7
    w0c, b0c = [t.to(dev) for t in ops.center_linear(w0, b0)]
    g, bt = (1.0 + _rand(84, (hid,), 0.2)).to(dev), _rand(85, (hid,), 0.2).to(dev)
    w3, b3 = _rand(86, (n, hid), hid ** -0.5).to(dev), _rand(87, (n,), 0.1).to(dev)
    res = _rand(88, (m, n)).to(dev)
    _clear(dev)
    with ops.act_scale_scope(s):
        got = ops.mlp_tail(x, w0c, b0c, g, bt, w3, b3, residual=res)
    _no_flag(dev)
    xd, w0d = x.double(), w0c.double()
    h = xd @ w0d.t() + b0c.double()
    eh = _gemm_bound(xd, w0d, s, ops.split_weight(w0c)[2], h)
    rstd = 1.0 / torch.sqrt(h.pow(2).mean(1, keepdim=True) + 1e-5)
    hn = h * rstd
    t = hn * g.double() + bt.double()
    a = torch.nn.functional.gelu(t)
    # LayerNorm + GELU in fp32 inside the staging: |dGELU| <= 1.13, the normalisation carries h's error relative to its spread,
    # fp32 arithmetic and the fitted Gaussian tail 2^-21 (|t| + 1)
    ea = 1.13 * g.double().abs() * rstd * eh.max(1, keepdim=True).values * (1.0 + hn.abs()) + 2.0 ** -21 * (t.abs() + 1.0)
    want = a @ w3.double().t() + b3.double() + res.double()
    bound = _gemm_bound(a, w3.double(), s, ops.split_weight(w3)[2], want) + ea @ w3.double().abs().t() + 2.0 ** -23 * res.double().abs()
    _worst("mlp_tail (lngelu)", s, (got.double() - want).abs(), bound, log)
    # ---- 3x3 convolution + F.normalize over the channels in the epilogue (Cout <= 128)
    B, Hh, Ww, cin, cout = 1, 21, 27, 64, 128
    xc = _logu(91, (B, Hh, Ww, cin), s).to(dev)
    wc, bc = _rand(92, (cout, 3, 3, cin), (9 * cin) ** -0.5).to(dev), _rand(93, (cout,), 0.1).to(dev)
    with ops.act_scale_scope(s):
        yc = ops.conv2d_nhwc(xc, wc, bc, ks=3, precision="x3", l2norm=True)
    _no_flag(dev)
    xn, wn = xc.double().permute(0, 3, 1, 2), wc.double().permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xn, wn, bc.double(), padding=1)
    ay = torch.nn.functional.conv2d(xn.abs(), wn.abs(), padding=1)
    ones = torch.nn.functional.conv2d(torch.ones_like(xn), wn.abs(), padding=1)
    ey = C * (2.0 ** -21 * ay + 2.0 ** -25 / s * ones) + 2.0 ** -23 * y.abs()
    nrm = y.pow(2).sum(1, keepdim=True).sqrt()
    want = (y / nrm).permute(0, 2, 3, 1)
    # x / ||x||: the error of one channel plus its share of the norm's, + fp32 normalisation
    bound = (ey / nrm + ey.pow(2).sum(1, keepdim=True).sqrt() / nrm).permute(0, 2, 3, 1) + 2.0 ** -21
    _worst("conv + l2norm", s, (yc.double() - want).abs(), bound, log)
    # ---- sfd2_conv1: conv1a (3 -> 64, image staged at s) -> BN -> ReLU -> split at s -> conv1b (stride 2) -> BN -> ReLU
    img = _logu(101, (1, 3, 29, 35), s).to(dev)
    wa, wb = _rand(102, (64, 3, 3, 4), 0.2).to(dev), _rand(103, (64, 3, 3, 64), 576 ** -0.5).to(dev)
    wa[..., 3] = 0.0
    ba, sa, ta = _rand(104, (64,), 0.1).to(dev), (1.0 + _rand(105, (64,), 0.1)).to(dev), _rand(106, (64,), 0.1).to(dev)
    bb, sb, tb = _rand(107, (64,), 0.1).to(dev), (1.0 + _rand(108, (64,), 0.1)).to(dev), _rand(109, (64,), 0.1).to(dev)
    with ops.act_scale_scope(s):
        c1 = ops.sfd2_conv1(img, wa, ba, sa, ta, wb, bb, sb, tb)
    _no_flag(dev)
    imd = img.double()
    wad, wbd = wa.double().permute(0, 3, 1, 2)[:, :3], wb.double().permute(0, 3, 1, 2)
    bn = lambda t, sc, sh: t * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    za = torch.nn.functional.conv2d(imd, wad, ba.double(), padding=1)
    y1 = torch.relu(bn(za, sa, ta))
    e1 = sa.double().abs()[None, :, None, None] * (C * (2.0 ** -21 * torch.nn.functional.conv2d(imd.abs(), wad.abs(), padding=1)
                                                       + 2.0 ** -25 / s * torch.nn.functional.conv2d(torch.ones_like(imd), wad.abs(), padding=1))
                                                  + 2.0 ** -23 * za.abs()) + 2.0 ** -23 * y1
    zb = torch.nn.functional.conv2d(y1, wbd, bb.double(), padding=1, stride=2)
    want = torch.relu(bn(zb, sb, tb)).permute(0, 2, 3, 1)
    eb = C * (2.0 ** -21 * torch.nn.functional.conv2d(y1, wbd.abs(), padding=1, stride=2)
              + 2.0 ** -25 / s * torch.nn.functional.conv2d(torch.ones_like(y1), wbd.abs(), padding=1, stride=2)) \
        + torch.nn.functional.conv2d(e1, wbd.abs(), padding=1, stride=2) + 2.0 ** -23 * zb.abs()
    bound = (sb.double().abs()[None, :, None, None] * eb).permute(0, 2, 3, 1) + 2.0 ** -23 * want
    _worst("sfd2_conv1", s, (c1.double() - want).abs(), bound, log)
    print("; ".join(log))


@pytest.mark.parametrize("s", SCALES)
def test_attention_accuracy_against_fp64(dev, s, attn_modes):
    """attention_x3 on planes at scale s: values spanning every regime of the split; queries / keys up to 2^2 (logits of O(10):
    beyond that the soft-max is an arg-max and the bound below says nothing).  Bound: the value planes' error weighted by the
    probabilities, the logits' error (a split product over both planes' floors, times scale) moving the output by at most
    twice its size times max |v|, and the probabilities' own two-part fp16 rounding."""
    S, T, hd = 1, 320, 4
    q, k = _logu(111, (T, hd * 64), s, hi=0.0), _logu(112, (T, hd * 64), s, hi=0.0)
    v = _logu(113, (T, hd * 64), s)
    scale = 0.125
    qp, kp, vp = _planes(q, s), _planes(k, s), _planes(v, s)
    vt = ops.value_planes_t(tuple(t.to(dev) for t in vp), S, hd, T)
    _clear(dev)
    with ops.act_scale_scope(s):
        o = ops.attention_x3(tuple(t.to(dev) for t in qp), tuple(t.to(dev) for t in kp), vt, S, hd, T, T, scale)
    _no_flag(dev)
    qd, kd, vd = (t.double().view(T, hd, 64).transpose(0, 1) for t in (q, k, v))
    p = torch.softmax(qd @ kd.transpose(1, 2) * scale, -1)
    want = (p @ vd).transpose(0, 1).reshape(T, hd * 64)
    pv = (p @ vd.abs()).transpose(0, 1).reshape(T, hd * 64)
    dl = scale * C * (2.0 ** -21 * (qd.abs() @ kd.abs().transpose(1, 2)) + 2.0 ** -25 / s * (qd.abs().sum(-1, keepdim=True) + kd.abs().sum(-1)[:, None, :]))
    dmax = dl.max(-1).values.transpose(0, 1).repeat_interleave(64, 1)       # per (query, head)
    vmax = float(vd.abs().max())
    bound = C * (2.0 ** -21 * pv + 2.0 ** -25 / s) + torch.expm1(2.0 * dmax) * vmax + 2.0 ** -20 * pv + 2.0 ** -23 * want.abs()
    d = (o.cpu().double() - want).abs()
    r = float((d / bound).max())
    print(f"attention s=2^{int(math.log2(s))}: max|err| {float(d.max()):.2e}, max err/bound {r:.3f}")
    assert r <= 1.0


# ================================================================================================ 3. the range edge
def _edge(dev, run, s, want=None, tol=None):
    """run(value) -> fp32 result(s); value = 65504 / s must pass (no flag, finite, fp32-class), 65520 / s must set the flag"""
    _clear(dev)
    with ops.act_scale_scope(s):
        got = run(65504.0 / s)
    assert not ops.x3_range_exceeded(dev), ("flag at 65504", s)
    if want is not None:
        g, w_ = got.double(), want(65504.0 / s)
        assert bool(torch.isfinite(g).all())
        err = float((g - w_).abs().max() / w_.abs().max())
        assert err < tol, (s, err)
    with ops.act_scale_scope(s):
        run(65520.0 / s)
    assert ops.x3_range_exceeded(dev), ("no flag at 65520", s)


@pytest.mark.parametrize("s", SCALES)
def test_range_edge_at_every_plane_writing_site(dev, s):
    """|s x| = 65504 (the largest fp16) is carried, 65520 (rounds to inf) is reported, at every site that splits a value:
    linear staging and its plane epilogue, the qkv epilogue (q / k column and value column), the LayerNorm + GELU staging,
    convolution staging and its plane epilogue, sfd2_conv1's image and its conv1a intermediate, GML's matching-descriptor planes"""
    tol = 2.0 ** -19                                 # relative to the largest |result|: fp32 class
    m, k, n = 192, 256, 192
    x = _rand(121, (m, k)).to(dev)
    w = _rand(122, (n, k), k ** -0.5).to(dev)
    b = _rand(123, (n,), 0.1).to(dev)
    ref = x.double() @ w.double().t() + b.double()

    def stage(v):
        xx = x.clone()
        xx[77, 5] = -v
        return ops.linear(xx, w, b, precision="x3")

    def stage_ref(v):
        xx = x.double().clone()
        xx[77, 5] = -v
        return xx @ w.double().t() + b.double()
    _edge(dev, stage, s, stage_ref, tol)
    # plane epilogue: output column 7 is its bias alone (zero weight row) — the staging sees in-range data
    wz = w.clone()
    wz[7] = 0.0

    def epi(v, alpha=1.0):
        bb = b.clone()
        bb[7] = v / alpha
        y, pl = ops.linear(x, wz, bb, alpha=alpha, split_out="also", precision="x3")
        return torch.stack([y, (pl[0].float() + pl[1].float()) / s]) if bool(torch.isfinite(pl[0].float()).all()) else y[None]

    def epi_ref(v, alpha=1.0):
        bb = b.double().clone()
        bb[7] = v / alpha
        y = alpha * (x.double() @ wz.double().t() + bb)
        return torch.stack([y, y])
    _edge(dev, epi, s, epi_ref, tol)
    # GML's matching-descriptor planes: ops.linear(..., alpha = 1 / d^0.25, split_out="only") (nets/gml.py)
    _edge(dev, lambda v: epi(v, 256 ** -0.25), s, lambda v: epi_ref(v, 256 ** -0.25), tol)
    # qkv epilogue: q / k column 9 and value column 128 + 50 (heads = 1: columns 128..191 are the values).  The value planes
    # are transposed and key-permuted: compared per column as sorted sets of values.
    for col in (9, 128 + 50):
        wq = w.clone()
        wq[col] = 0.0

        def qkv(v, col=col):
            bb = b.clone()
            bb[col] = v
            pl, vt = ops.linear_qkv_planes(x, wq, bb, 1, m)
            vals = _val(vt, s)[0, 0].t()
            if not bool(torch.isfinite(vals).all()):
                return vals
            return torch.cat([_val(pl, s), vals.sort(0).values], 1)

        def qkv_ref(v, col=col):
            bb = b.double().clone()
            bb[col] = v
            y = x.double() @ wq.double().t() + bb
            return torch.cat([y[:, :128], y[:, 128:].sort(0).values], 1)
        _edge(dev, qkv, s, qkv_ref, tol)
    # LayerNorm + GELU staging: gamma 0 and a large beta make one hidden column exactly beta after GELU (GELU(t) = t beyond 6)
    hid = 256
    w0c, b0c = [t.to(dev) for t in ops.center_linear(_rand(124, (hid, k), k ** -0.5), _rand(125, (hid,), 0.3))]
    g, bt = (1.0 + _rand(126, (hid,), 0.2)).to(dev), _rand(127, (hid,), 0.2).to(dev)
    w3, b3 = _rand(128, (n, hid), hid ** -0.5 * 2.0 ** -10).to(dev), _rand(129, (n,), 0.1).to(dev)

    def tail(v):
        gg, bb = g.clone(), bt.clone()
        gg[11], bb[11] = 0.0, v
        return ops.mlp_tail(x, w0c, b0c, gg, bb, w3, b3)

    def tail_ref(v):
        h = x.double() @ w0c.double().t() + b0c.double()
        gg, bb = g.double().clone(), bt.double().clone()
        gg[11], bb[11] = 0.0, v
        a = torch.nn.functional.gelu(torch.nn.functional.layer_norm(h, (hid,), gg, bb, 1e-5))
        return a @ w3.double().t() + b3.double()
    _edge(dev, tail, s, tail_ref, 2.0 ** -17)
    # convolution staging and its plane epilogue
    xc = _rand(131, (1, 13, 17, 64)).to(dev)
    wc = _rand(132, (64, 3, 3, 64), 576 ** -0.5).to(dev)
    bc = _rand(133, (64,), 0.1).to(dev)
    conv_ref = lambda xx, ww, bb: torch.nn.functional.conv2d(xx.double().permute(0, 3, 1, 2), ww.double().permute(0, 3, 1, 2), bb.double(),
                                                             padding=1).permute(0, 2, 3, 1)

    def cstage(v):
        xx = xc.clone()
        xx[0, 6, 9, 33] = v
        return ops.conv2d_nhwc(xx, wc, bc, ks=3, precision="x3")

    def cstage_ref(v):
        xx = xc.clone()
        xx[0, 6, 9, 33] = v
        return conv_ref(xx, wc, bc)
    _edge(dev, cstage, s, cstage_ref, tol)
    wz = wc.clone()
    wz[21] = 0.0

    def cplanes(v):
        bb = bc.clone()
        bb[21] = v
        return _val(ops.conv2d_nhwc_planes(xc, wz, bb, ks=3), s)

    def cplanes_ref(v):
        bb = bc.clone()
        bb[21] = v
        return conv_ref(xc, wz, bb)
    _edge(dev, cplanes, s, cplanes_ref, tol)
    # sfd2_conv1: an image pixel, and conv1a's output channel 5 (zero weights, bias alone) on its way into conv1b
    img = _rand(141, (1, 3, 21, 25)).to(dev)
    wa, wb = _rand(142, (64, 3, 3, 4), 0.2).to(dev), _rand(143, (64, 3, 3, 64), 576 ** -0.5 * 2.0 ** -10).to(dev)
    wa[..., 3] = 0.0
    one, zero = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    ba, bb = _rand(144, (64,), 0.1).to(dev), _rand(145, (64,), 0.1).to(dev)

    wat = wa * 2.0 ** -12      # the image pixel's conv1a outputs stay inside the range: the image's own split is the site

    def c1_ref(im, wa_, ba_):
        y1 = torch.relu(torch.nn.functional.conv2d(im.double(), wa_.double().permute(0, 3, 1, 2)[:, :3], ba_.double(), padding=1))
        return torch.relu(torch.nn.functional.conv2d(y1, wb.double().permute(0, 3, 1, 2), bb.double(), padding=1, stride=2)).permute(0, 2, 3, 1)

    def c1_img(v):
        im = img.clone()
        im[0, 1, 10, 12] = v
        return ops.sfd2_conv1(im, wat, ba, one, zero, wb, bb, one, zero)

    def c1_img_ref(v):
        im = img.clone()
        im[0, 1, 10, 12] = v
        return c1_ref(im, wat, ba)
    _edge(dev, c1_img, s, c1_img_ref, tol)
    wa5 = wa.clone()
    wa5[5] = 0.0

    def c1_mid(v):
        b_ = ba.clone()
        b_[5] = v
        return ops.sfd2_conv1(img, wa5, b_, one, zero, wb, bb, one, zero)

    def c1_mid_ref(v):
        b_ = ba.clone()
        b_[5] = v
        return c1_ref(img, wa5, b_)
    _edge(dev, c1_mid, s, c1_mid_ref, tol)


# ================================================================================================ 4. models at every guard scale
def _adagml(dev):
    from pram_amd.nets.adagml import AdaGML
    a = AdaGML({})
    a.load_state_dict(H.adagml_sd(), strict=True)
    return a.to(dev).eval()


@pytest.mark.parametrize("scale", LADDER)
def test_adagml_and_sc_head_at_every_guard_scale(dev, golden, scale):
    """AdaGML (its pruning decisions come from split-fp16 logits) against its golden vectors: stop layer, survivor ids and match
    indices exact, scores within 1e-3; SegNetViT with the sc head within 1e-3 — at every scale the range guard can leave them"""
    g = golden("adagml_m300_n280")
    data, _ = H.pair_data(int(g["pair_index"]), int(g["m"]), int(g["n"]), device=dev)
    net = _adagml(dev).set_act_scale(scale)
    probes = {}
    r = net.produce_matches(data, p=0.0, probes=probes)
    lens = probes["lens"].tolist()
    ds = float(np.abs(r["matching_scores0"].cpu().numpy() - g["s0"]).max())
    print(f"adagml s={scale:g}: stop {int(probes['stop_layer'][0])}, survivors {lens}, |score - golden| {ds:.2e}")
    assert int(probes["stop_layer"][0].item()) == int(g["stop_layer"])
    assert np.array_equal(probes["ind"][0, :lens[0]].cpu().numpy(), g["ind0"]) and np.array_equal(probes["ind"][1, :lens[1]].cpu().numpy(), g["ind1"])
    assert np.array_equal(r["matches0"].cpu().numpy(), g["m0_p0"]) and ds < 1e-3
    from pram_amd.nets.segnetvit import SegNetViT
    g = golden("segnetvit_with_sc")
    m = SegNetViT({"n_class": int(g["n_class"]), "n_layers": int(g["n_layers"]), "with_sc": True})
    m.load_state_dict(W.make_state_dict("segnetvit", m.state_dict(), seed=7), strict=True)
    m = m.to(dev).eval().set_act_scale(scale)
    d0, k0 = W.synthetic_tokens(9, int(g["N"]))[:2]
    out = m({"seg_descriptors": d0[None].to(dev), "keypoints": k0[None].to(dev), "image": torch.empty(1, 3, 480, 640)})
    dsc = float(np.abs(out["sc"].cpu().numpy() - g["sc"]).max())
    dpr = float(np.abs(out["prediction"][:, :8].cpu().numpy() - g["prediction_rows"]).max())
    print(f"segnetvit sc head s={scale:g}: |sc - golden| {dsc:.2e}, |logits - golden| {dpr:.2e}")
    assert dsc < 1e-3 and dpr < 1e-3
    assert ops.current_act_scale() == 16.0 and not ops.x3_range_exceeded(dev)


def test_c5_fp16_path_at_the_lowest_guard_scale(dev):
    """BASELINE C5 (fp16 MFMA path) keeps split-fp16 kernels of its own (GML's matching descriptors): at ACT_SCALE_MIN the
    recogniser and the matcher stay within the frozen bench.F16_BARS"""
    import bench
    from pram_amd.nets.gml import GML
    from pram_amd.nets.load_segnet import load_segnet
    desc, kp = W.synthetic_tokens(2, 2048)[:2]
    ref = R.segnetvit_forward(H.segnet_sd(113), desc[None], kp[None], (1, 3, 480, 640))
    seg = load_segnet('segnetvit', 113, 256, 15, 1024)
    seg.load_state_dict(H.segnet_sd(113), strict=True)
    seg = seg.to(dev).eval().set_precision("f16").set_act_scale(ops.ACT_SCALE_MIN)
    out = seg({"seg_descriptors": desc[None].to(dev), "keypoints": kp[None].to(dev), "image": torch.empty(1, 3, 480, 640)})["prediction"]
    d = H.maxdiff(out, ref)
    agree = (out.argmax(-1).cpu() == ref.argmax(-1)).float().mean().item()
    data, _ = H.pair_data(0, 1024, 1024)
    refm = R.gml_produce_matches(H.gml_sd(), data, p=0.0)
    gml = GML({})
    gml.load_state_dict(H.gml_sd(), strict=True)
    gml = gml.to(dev).eval().set_precision("f16").set_act_scale(ops.ACT_SCALE_MIN)
    _clear(dev)
    rm = gml.produce_matches({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}, p=0.0)
    magree = (rm["matches0"].cpu() == refm["matches0"]).float().mean().item()
    print(f"C5 at s={ops.ACT_SCALE_MIN:g}: logits {d:.2e}, arg-max {agree:.4f}, match agreement {magree:.4f}")
    assert d < bench.F16_BARS["logits"] and agree >= bench.F16_BARS["argmax"] and magree >= bench.F16_BARS["match_agree"]
    assert not ops.x3_range_exceeded(dev)


# ================================================================================================ 5. the guard's descent in a pipeline
def test_guard_descends_the_whole_ladder_inside_a_pipeline(dev):
    """SFD2 + a SegNetViT whose residual stream needs ACT_SCALE_MIN (|x| in [65520 / (16 MIN), 65520 / MIN)) + GML, one run
    under the default policy: the guard walks every step of the ladder, lowers EVERY model that ran (it cannot tell which one
    tripped), stays on the split kernels — and the extractor, the matcher and the recogniser keep their bars against the same
    run on the exact-fp32 kernels"""
    from pram_amd.nets.gml import GML
    from pram_amd.nets.sfd2 import ResNet4x
    from pram_amd.nets.load_segnet import load_segnet
    from pram_amd.pipeline import QueryPipeline
    sfd2 = ResNet4x()
    sfd2.load_state_dict(H.sfd2_sd(), strict=True)
    sfd2 = sfd2.to(dev).eval()
    gml = GML({})
    gml.load_state_dict(H.gml_sd(), strict=True)
    gml = gml.to(dev).eval()
    # the residual stream of this SegNetViT peaks at ~1.2 x gain (seed-7 weights): aim at the middle of the band (in octaves)
    gain = 65520.0 / (4.0 * ops.ACT_SCALE_MIN) / 1.2
    sd = dict(H.segnet_sd())
    sd["input_proj.weight"] = sd["input_proj.weight"] * gain
    sd["input_proj.bias"] = sd["input_proj.bias"] * gain
    seg = load_segnet('segnetvit', 113, 256, 15, 1024)
    seg.load_state_dict(sd, strict=True)
    seg = seg.to(dev).eval()
    img = torch.stack([W.synthetic_image(1, 96, 128), W.synthetic_image(2, 96, 128)]).to(dev)
    pipe = QueryPipeline(sfd2, seg, gml, max_keypoints=128, min_keypoints=8)
    ex = sfd2.extract_batched(img, pipe.cfg)
    ref = {"descriptors": ex["descriptors"].flip(1).contiguous(), "keypoints": ex["keypoints"].flip(1).contiguous(),
           "scores": ex["scores"].flip(1).contiguous()}
    assert sfd2.act_scale == seg.act_scale == gml.act_scale == 16.0
    _clear(dev)
    ev = dict(ops.guard_events)
    out = pipe.run(img, ref, stages="erm")
    assert ops.guard_events["rescaled"] == ev["rescaled"] + len(LADDER) - 1, "fixture must need the lowest scale"
    assert ops.guard_events["f32_fallback"] == ev["f32_fallback"]
    assert sfd2.act_scale == seg.act_scale == gml.act_scale == ops.ACT_SCALE_MIN
    with ops.forced_precision("f32"):
        want = pipe.run(img, ref, stages="erm")
    worst = {"desc": 0.0, "score": 0.0, "logit_rel": 0.0}
    for b in range(img.shape[0]):
        n = int(want["counts"][b])
        assert int(out["counts"][b]) == n
        kg = {tuple(p) for p in out["keypoints"][b, :n].cpu().tolist()}
        kw = {tuple(p) for p in want["keypoints"][b, :n].cpu().tolist()}
        assert kg == kw, f"frame {b}: keypoint sets differ ({len(kg ^ kw)})"
        worst["desc"] = max(worst["desc"], H.maxdiff(out["descriptors"][b, :n], want["descriptors"][b, :n]))
        assert torch.equal(out["matches0"][b], want["matches0"][b]), f"frame {b}: match indices differ"
        worst["score"] = max(worst["score"], H.maxdiff(out["matching_scores0"][b], want["matching_scores0"][b]))
        peak = float(want["prediction"][b, :n].abs().max())
        worst["logit_rel"] = max(worst["logit_rel"], H.maxdiff(out["prediction"][b, :n], want["prediction"][b, :n]) / peak)
    print(f"pipeline at s={ops.ACT_SCALE_MIN:g} vs exact fp32: {worst}")
    assert worst["desc"] <= 1e-3 and worst["score"] <= 1e-3 and worst["logit_rel"] <= 1e-4, worst
