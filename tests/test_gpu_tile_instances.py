"""GPU (MI355X): every kernel instantiation the launch grid can select (tests/tile_instances.py), each at a shape that reaches it.

A case (1) asserts that the library launched the instantiation the table names (ops.last_kernel()), (2) compares the result
with an fp64 reference on the operands the kernel consumes, under the bar the existing test of that path uses, and (3) runs a
slice of the problem through the same entry on a small grid — another instantiation — and compares the shared rows: equal bits
where the sources promise them (eight- / four-wave and chunked attention, halo / wide / narrow split-fp16 convolutions, the
row sums of squares of the MLP tail), err_big <= 2 * err_small + 1e-7 elsewhere (the same products in another grouping; a
row or column mapped to the wrong accumulator register gives errors of order 1).  Every case prints one 'TILE' line."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from pram_amd import ops
from tests import tile_instances as TI

pytestmark = pytest.mark.gpu

HEADS = 4


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def gen(dev, key, shape, std=1.0):
    g = torch.Generator(device=dev)
    g.manual_seed(zlib.crc32(key.encode()))
    return torch.randn(shape, generator=g, device=dev) * std


def planes(t2d):
    """fp32 -> (hi, lo) fp16 planes of t * 16, and the value they carry in fp64"""
    s = t2d * 16.0
    hi = s.half()
    lo = (s - hi.float()).half()
    return (hi.contiguous(), lo.contiguous()), (hi.double() + lo.double()) / 16.0


def is_small(tag):
    """the instantiation a small grid gets (or the only one there is)"""
    return "<1," in tag or "cin4" in tag or tag.endswith("w4,interleaved>") or tag == "attention_h16t<4>"


def maxerr(a, ref64):
    return float((a.double() - ref64).abs().max()) if a.numel() else 0.0


class Report:
    """the comparison of a case's shared rows with its small launches; prints the case's line"""

    def __init__(self, c):
        self.c, self.eb, self.es, self.small_tags, self.equal = c, 0.0, 0.0, set(), True

    def shared(self, big_rows, small, small_tag, ref_rows, promise):
        c = self.c
        if small_tag == c["tag"]:
            assert is_small(c["tag"]), f"the slice landed on the case's own instantiation {small_tag}"
            return
        self.small_tags.add(small_tag)
        eb, es = maxerr(big_rows, ref_rows), maxerr(small, ref_rows)
        self.eb, self.es = max(self.eb, eb), max(self.es, es)
        eq = torch.equal(big_rows, small)
        self.equal = self.equal and eq
        if promise:
            assert eq, f"{c['tag']} and {small_tag} promise equal bits: max |d| {maxerr(big_rows, small.double()):.3e}"
        assert eb <= 2 * es + 1e-7, (c["tag"], small_tag, eb, es)

    def done(self, err_full):
        c = self.c
        bar, where = TI.BARS[c["bar"]]
        print(f"TILE {TI.case_id(c)}: tag {c['tag']} small {'|'.join(sorted(self.small_tags)) or '-'} err_full {err_full:.2e} "
              f"err_big {self.eb:.2e} err_small {self.es:.2e} bits_equal {self.equal if self.small_tags else '-'} bar {bar:g}")
        assert err_full < bar, (err_full, bar, where)


def tag_is(want):
    got = ops.last_kernel()
    assert got == want, f"launched {got}, the table says {want}"


def ends(m, rows=128):
    return [slice(0, rows), slice(m - rows, m)] if m > rows else []


LENS_PATTERN = (1.0, 0.0, 1.0 / 64, 0.58, 0.33)


def ragged_lens(dev, seqs, t):
    return torch.tensor([max(int(LENS_PATTERN[i % 5] * t), 1 if LENS_PATTERN[i % 5] else 0) for i in range(seqs)], dtype=torch.int32, device=dev)


def row_mask(lens, t):
    return (torch.arange(lens.numel() * t, device=lens.device) % t) < lens.repeat_interleave(t)


def rotary_ref(v, cos, sin):
    """the epilogue's rotation of the first 64 columns: column r pairs with column 32 + r"""
    v = v.clone()
    v0, v1, c, s = v[:, :32].clone(), v[:, 32:64].clone(), cos.double(), sin.double()
    v[:, :32] = v0 * c - v1 * s
    v[:, 32:64] = v1 * c + v0 * s
    return v


# ------------------------------------------------------------------------------------------------ linear
def run_linear(dev, c, rep):
    m, n, k, epi, prec = c["m"], c["n"], c["k"], c["epi"], c["prec"]
    t_pad = 1024
    if epi == "lens":
        m = -(-m // t_pad) * t_pad
    k0, k1 = (k // 2, k // 2) if epi == "x2" else (k, 0)
    key = TI.case_id(c)
    x, x2 = gen(dev, key + "x", (m, k0)), gen(dev, key + "x2", (m, k1)) if k1 else None
    w, b = gen(dev, key + "w", (n, k), k ** -0.5), gen(dev, key + "b", (n,), 0.1)
    res, alpha = (gen(dev, key + "r", (m, n)), 0.25) if epi == "bias_res_alpha" else (None, 1.0)
    cos = sin = None
    if epi == "rotary":
        ang = gen(dev, key + "ang", (m, 32), 1.7)
        cos, sin = torch.cos(ang), torch.sin(ang)

    def call(rows, **extra):
        kw = dict(x2=None if x2 is None else x2[rows], residual=None if res is None else res[rows], alpha=alpha, precision=prec, **extra)
        if cos is not None:
            kw["rotary"] = (cos[rows], sin[rows], 64)
        if epi == "split_also":
            out, pl = ops.linear(x[rows], w, b, split_out="also", **kw)
            return out, pl, ops.last_kernel()
        return ops.linear(x[rows], w, b, **kw), None, ops.last_kernel()

    xa = x if x2 is None else torch.cat([x, x2], 1)
    xd, wd = (xa.half().double(), w.half().double()) if prec == "f16" else (xa.double(), w.double())
    ref = (xd @ wd.t() + b.double()) * alpha
    if cos is not None:
        ref = rotary_ref(ref, cos, sin)
    if res is not None:
        ref = ref + res.double()
    out, pl, tag = call(slice(0, m))
    assert tag == c["tag"], f"launched {tag}, the table says {c['tag']}"
    if pl is not None:      # hi + lo = 16 x the fp32 result to 2^-21 relative (2^-29 absolute below 2^-7)
        rel_bar = TI.BARS["planes_rel"][0]
        rec, o64 = (pl[0].double() + pl[1].double()) / 16.0, out.double()
        d, big = (rec - o64).abs(), o64.abs() >= 2.0 ** -7
        assert float((d[big] / o64.abs()[big]).max()) < rel_bar and float(d[~big].max()) <= 2.0 ** -29
    if epi == "lens":       # untouched rows keep the sentinel, valid rows are the dense call's bits
        lens = ragged_lens(dev, m // t_pad, t_pad)
        rag = torch.full((m, n), 3.0, device=dev)
        ops.linear(x, w, b, precision=prec, out=rag, lens=lens, t_pad=t_pad)
        tag_is(c["tag"])
        valid = row_mask(lens, t_pad)
        assert torch.equal(rag[valid], out[valid]) and bool((rag[~valid] == 3.0).all())
    for rows in ends(m):
        small, _, stag = call(rows)
        rep.shared(out[rows], small, stag, ref[rows], promise=False)
    rep.done(maxerr(out, ref))


def run_linear_planes(dev, c, rep):
    m, n, k, epi = c["m"], c["n"], c["k"], c["epi"]
    k0, k1 = (k // 2, k // 2) if epi == "x2" else (k, 0)
    key = TI.case_id(c)
    px, xv = planes(gen(dev, key + "x", (m, k0)))
    px2, x2v = planes(gen(dev, key + "x2", (m, k1))) if k1 else (None, None)
    w, b = gen(dev, key + "w", (n, k), k ** -0.5), gen(dev, key + "b", (n,), 0.1)
    res, alpha = (gen(dev, key + "r", (m, n)), 0.25) if epi == "bias_res_alpha" else (None, 1.0)

    def call(rows):
        out = ops.linear_planes((px[0][rows], px[1][rows]), w, b, x2=None if px2 is None else (px2[0][rows], px2[1][rows]),
                                residual=None if res is None else res[rows], alpha=alpha)
        return out, ops.last_kernel()

    xa = xv if x2v is None else torch.cat([xv, x2v], 1)
    ref = (xa @ w.double().t() + b.double()) * alpha
    if res is not None:
        ref = ref + res.double()
    out, tag = call(slice(0, m))
    assert tag == c["tag"], f"launched {tag}, the table says {c['tag']}"
    for rows in ends(m):
        small, stag = call(rows)
        rep.shared(out[rows], small, stag, ref[rows], promise=False)
    rep.done(maxerr(out, ref))


def run_linear_qkv_planes(dev, c, rep):
    m, n, k, heads, t = c["m"], c["n"], c["k"], c["heads"], c["t_seq"]
    col0, seqs = n - heads * 64, m // t
    key = TI.case_id(c)
    x, w, b = gen(dev, key + "x", (m, k)), gen(dev, key + "w", (n, k), k ** -0.5), gen(dev, key + "b", (n,), 0.1)
    ang = gen(dev, key + "ang", (m, 32), 1.7)
    cos, sin = torch.cos(ang), torch.sin(ang)
    lens = ragged_lens(dev, seqs, t)
    valid = row_mask(lens, t)
    ref = rotary_ref(x.double() @ w.double().t() + b.double(), cos, sin)
    pq, vt = ops.linear_qkv_planes(x, w, b, heads, t, rotary=(cos, sin, 64), lens=lens)
    tag_is(c["tag"])
    # the same projection as row-major planes (the split_out epilogue) and the transposition kernel: equal bits
    _, pl = ops.linear(x, w, b, rotary=(cos, sin, 64), split_out="only", lens=lens, t_pad=t, precision="x3")
    tag_is(c["tag"])
    vt_ref = ops.value_planes_t((pl[0][:, col0:], pl[1][:, col0:]), seqs, heads, t, lens)
    some = lens > 0      # whole 64-token blocks without a valid token are never read
    for i in (0, 1):
        assert torch.equal(pq[i][valid], pl[i][valid, :col0])
        assert torch.equal(vt[i][some], vt_ref[i].view(seqs, heads, 64, t)[some])
    # against fp64: the planes carry the fp32 result to 2^-21 relative on top of the GEMM's own bar
    bar = TI.BARS[c["bar"]][0]
    rec_all = (pl[0].double() + pl[1].double()) / 16.0
    excess = (rec_all[valid] - ref[valid]).abs() - 2.0 ** -21 * ref[valid].abs()
    assert float(excess.max()) < bar, float(excess.max())
    rec = (pq[0].double() + pq[1].double()) / 16.0
    for rows in ends(m):
        (sh, sl), _ = ops.linear_qkv_planes(x[rows], w, b, heads, t, rotary=(cos[rows], sin[rows], 64), lens=lens[rows.start // t:rows.stop // t].contiguous())
        stag = ops.last_kernel()
        v = valid[rows]
        rep.shared(rec[rows][v], ((sh.double() + sl.double()) / 16.0)[v], stag, ref[rows][v][:, :col0], promise=False)
    rep.done(max(float(excess.max()), 0.0))


def run_mlp_tail(dev, c, rep):
    m, k, hid, n = c["m"], c["k"], c["hid"], c["n"]
    key = TI.case_id(c)
    L = ops._lib.load()
    x = gen(dev, key + "x", (m, k))
    w0, b0 = gen(dev, key + "w0", (hid, k), k ** -0.5), gen(dev, key + "b0", (hid,), 0.3) + 0.7
    g, bt = 1.0 + gen(dev, key + "g", (hid,), 0.2), gen(dev, key + "bt", (hid,), 0.2)
    w3, b3 = gen(dev, key + "w3", (n, hid), hid ** -0.5), gen(dev, key + "b3", (n,), 0.1)
    res = gen(dev, key + "r", (m, n))
    w0c, b0c = [t.to(dev) for t in ops.center_linear(w0, b0)]
    wh, wl, ws = ops.split_weight(w0c)
    parts = int(L.pram_linear_x3_ssq_parts(m, hid, k))

    def ssq_of(rows):
        xr = x[rows]
        h = torch.empty(xr.shape[0], hid, device=dev)
        ssq = torch.empty(parts, xr.shape[0], device=dev)
        ops._lib.check(L.pram_linear_x3_ssq_f32(xr.data_ptr(), k, k, None, 0, 0, wh.data_ptr(), wl.data_ptr(), ws, b0c.data_ptr(), h.data_ptr(), hid,
                                                ssq.data_ptr(), xr.shape[0], hid, None, 0, torch.cuda.current_stream().cuda_stream), "pram_linear_x3_ssq_f32")
        return ssq, ops.last_kernel()

    ssq, tag_first = ssq_of(slice(0, m))
    assert tag_first == c["tag_first"], f"first GEMM launched {tag_first}, the table says {c['tag_first']}"
    got = ops.mlp_tail(x, w0c, b0c, g, bt, w3, b3, residual=res)
    tag_is(c["tag"])
    hh = F.layer_norm(x.double() @ w0.double().t() + b0.double(), (hid,), g.double(), bt.double(), 1e-5)
    ref = F.gelu(hh) @ w3.double().t() + b3.double() + res.double()
    for rows in ends(m):
        ssq_s, stag_first = ssq_of(rows)
        if stag_first == tag_first:
            assert is_small(tag_first), f"the slice's first GEMM landed on the case's own instantiation {stag_first}"
        else:      # linear.hip: the partials are the same bits for every tile configuration
            assert torch.equal(ssq[:, rows], ssq_s), (tag_first, stag_first)
        small = ops.mlp_tail(x[rows], w0c, b0c, g, bt, w3, b3, residual=res[rows])
        rep.shared(got[rows], small, ops.last_kernel(), ref[rows], promise=False)
    rep.done(maxerr(got, ref))


def run_bgemm_nt(dev, c, rep):
    B, m, n, k = c["batch"], c["m"], c["n"], c["k"]
    key = TI.case_id(c)
    a, b = gen(dev, key + "a", (B, m, k), 0.5), gen(dev, key + "b", (B, n, k), 0.5)
    ref = torch.einsum("bmk,bnk->bmn", a.double(), b.double()) * 0.25
    out = ops.bgemm_nt(a, b, alpha=0.25)
    tag_is(c["tag"])
    for z in (0, B - 1):
        small = ops.bgemm_nt(a[z:z + 1], b[z:z + 1], alpha=0.25)
        rep.shared(out[z:z + 1], small, ops.last_kernel(), ref[z:z + 1], promise=False)
    rep.done(maxerr(out, ref))


def run_bgemm_nt_planes(dev, c, rep):
    B, m, n, k = c["batch"], c["m"], c["n"], c["k"]
    key = TI.case_id(c)
    pa, av = planes(gen(dev, key + "a", (B * m, k), 0.5))
    pb, bv = planes(gen(dev, key + "b", (B * n, k), 0.5))
    ref = torch.einsum("bmk,bnk->bmn", av.view(B, m, k), bv.view(B, n, k)) * 0.25
    out = ops.bgemm_nt_planes(pa, pb, B, m, n, alpha=0.25)
    tag_is(c["tag"])
    for z in (0, B - 1):
        small = ops.bgemm_nt_planes(tuple(p[z * m:(z + 1) * m] for p in pa), tuple(p[z * n:(z + 1) * n] for p in pb), 1, m, n, alpha=0.25)
        rep.shared(out[z:z + 1], small, ops.last_kernel(), ref[z:z + 1], promise=False)
    rep.done(maxerr(out, ref))


# ------------------------------------------------------------------------------------------------ convolutions
def conv_ref(x, w, bias, ks, stride):
    """NHWC x, OHWI w (already the values the kernel consumes, fp64) -> NHWC fp64, as im2col + matrix product"""
    B, H, W, cin = x.shape
    cout = w.shape[0]
    ho, wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    wm = w.permute(0, 3, 1, 2).reshape(cout, cin * ks * ks)
    out = torch.empty(B, ho, wo, cout, dtype=torch.float64, device=x.device)
    for i in range(B):
        cols = F.unfold(x[i:i + 1].permute(0, 3, 1, 2), ks, padding=ks // 2, stride=stride)[0]      # [cin * ks * ks][ho * wo]
        out[i] = (cols.t() @ wm.t() + bias).view(ho, wo, cout)
    return out


def run_conv(dev, c, rep):
    (B, H, W), cin, cout, ks, stride, prec, full = c["bhw"], c["cin"], c["cout"], c["ks"], c["stride"], c["prec"], c["form"] == "full"
    key = TI.case_id(c)
    x = gen(dev, key + "x", (B, H, W, cin))
    if cin == 4:
        x[..., 3] = 0.0      # the stem's padded RGB
    w, bias = gen(dev, key + "w", (cout, ks, ks, cin), (ks * ks * cin) ** -0.5), gen(dev, key + "b", (cout,), 0.1)
    xd, wd = (x.half().double(), w.half().double()) if prec == "f16" else (x.double(), w.double())
    ref = conv_ref(xd, wd, bias.double(), ks, stride)
    sc = sh = res = None
    if full:
        sc, sh = 1.0 + gen(dev, key + "s", (cout,), 0.1), gen(dev, key + "t", (cout,), 0.1)
        res = gen(dev, key + "r", tuple(ref.shape))
        ref = torch.relu(ref * sc.double() + sh.double() + res.double())
    out = ops.conv2d_nhwc(x, w, bias, sc, sh, residual=res, ks=ks, stride=stride, relu=full, precision=prec)
    tag_is(c["tag"])
    assert tuple(out.shape) == tuple(ref.shape)
    # conv.hip: the halo, the wide and the narrow split-fp16 kernels agree bit for bit
    promise = c["tag"].startswith(("conv_x3h", "conv_x3w"))

    def small_conv(band, res_band):
        return ops.conv2d_nhwc(band, w, bias, sc, sh, residual=None if res is None else res_band.contiguous(), ks=ks, stride=stride,
                               relu=full, precision=prec)

    # one tile band of the first image: input rows 0 .. 8 * stride + 1 give output rows 0 .. 7 exactly
    band = x[:1, :8 * stride + 2].contiguous()
    rows_s = (band.shape[1] + 2 * (ks // 2) - ks) // stride + 1
    small = small_conv(band, None if res is None else res[:1, :rows_s])
    rep.shared(out[:1, :8], small[:, :8], ops.last_kernel(), ref[:1, :8], promise)
    # ... and the last band of the last image (the ragged last row tile of the big launch): the input from row (ho - 9) * stride on
    # gives output rows ho - 9 .. ho - 1, all but the first of them (its upper neighbours are missing) exactly
    ho = out.shape[1]
    o0 = ho - 9
    small = small_conv(x[B - 1:, o0 * stride:].contiguous(), None if res is None else res[B - 1:, o0:])
    assert small.shape[1] == 9
    rep.shared(out[B - 1:, o0 + 1:], small[:, 1:], ops.last_kernel(), ref[B - 1:, o0 + 1:], promise)
    rep.done(maxerr(out, ref))


# ------------------------------------------------------------------------------------------------ attention
def attn_ref(q, k, v, scale):
    """q [mq, H * 64], k / v [nk, H * 64] fp64 -> [mq, H * 64]"""
    sp = lambda t: t.view(t.shape[0], HEADS, 64).transpose(0, 1)
    return (torch.softmax(sp(q) @ sp(k).transpose(1, 2) * scale, -1) @ sp(v)).transpose(0, 1).reshape(q.shape[0], HEADS * 64)


class attention_knobs:
    """the process-wide settings an attention case runs under, restored afterwards"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        L, c = ops._lib.load(), self.c
        self.chunk = L.pram_attention_x3_set_chunk_keys(0)
        self.ps = L.pram_attention_x3_set_p_split(-1)
        self.split = ops.attention_split
        L.pram_attention_x3_set_chunk_keys(c.get("chunk", 4096))
        L.pram_attention_x3_set_p_split(c.get("p_split", 1))
        self.target = L.pram_attention_x3_set_split_target(c.get("target", -1))
        ops.attention_split = c.get("split", True)

    def __exit__(self, *exc):
        L = ops._lib.load()
        L.pram_attention_x3_set_chunk_keys(self.chunk)
        L.pram_attention_x3_set_p_split(self.ps)
        L.pram_attention_x3_set_split_target(self.target)
        ops.attention_split = self.split


def run_attention(dev, c, rep):
    B, M, N, shift, h16 = c["batch"], c["m"], c["n"], c["kv_shift"], c["entry"] == "attention_h16t"
    key = TI.case_id(c)
    # operands of the test each bar is quoted from: q / k of deviation 1.2 beside unit values below 1024 keys (test_gpu_x3.py); from
    # there on the projections of unit tokens by weights of deviation 0.06 over K = 256 (test_gpu_guard_chunks_mlp.py): 0.96 for all
    # three.  The bars scale with them — a probability rounded to one fp16 moves the output by 2^-12 of the values' spread.
    sqk, sv = (1.2, 1.0) if N < 1024 else (0.96, 0.96)
    q, k, v = gen(dev, key + "q", (B * M, HEADS * 64), sqk), gen(dev, key + "k", (B * N, HEADS * 64), sqk), gen(dev, key + "v", (B * N, HEADS * 64), sv)
    qlens = [M - 37 * (i % 3) for i in range(B)]
    klens = [N - 13 * (i % 5) for i in range(B)]      # indexed by the key set
    ql, kl = torch.tensor(qlens, dtype=torch.int32, device=dev), torch.tensor(klens, dtype=torch.int32, device=dev)
    if h16:
        pq, pk, pv = q.half(), k.half(), v.half()
        qv, kv, vv = pq.double(), pk.double(), pv.double()
        vt = ops.value_t16(pv, B, HEADS, N, kl)
        call = lambda q_, k_, vt_, b_, ql_, kl_, sh_: ops.attention_h16t(q_, k_, vt_, b_, HEADS, M, N, 0.125, ql_, kl_, kv_shift=sh_)
        rows_of = lambda p, a, b: p[a:b]
        vt_of = lambda s: vt[s:s + 1].contiguous()
    else:
        (pq, qv), (pk, kv), (pv, vv) = planes(q), planes(k), planes(v)
        vt = ops.value_planes_t(pv, B, HEADS, N, kl)
        call = lambda q_, k_, vt_, b_, ql_, kl_, sh_: ops.attention_x3(q_, k_, vt_, b_, HEADS, M, N, 0.125, ql_, kl_, kv_shift=sh_)
        rows_of = lambda p, a, b: (p[0][a:b], p[1][a:b])
        vt_of = lambda s: tuple(t[s:s + 1].contiguous() for t in vt)
    with attention_knobs(c):
        out = call(pq, pk, vt, B, ql, kl, shift)
        tag_is(c["tag"])
        err = 0.0
        for s in range(B):
            ks_ = (s + shift) % B
            ref = attn_ref(qv[s * M:s * M + qlens[s]], kv[ks_ * N:ks_ * N + klens[ks_]], vv[ks_ * N:ks_ * N + klens[ks_]], 0.125)
            err = max(err, maxerr(out[s * M:s * M + qlens[s]], ref))
            if s in (1, B - 1):      # the sequence on its own, never through a workspace: attention_x3.hip promises the same bits
                ops.attention_split = False
                one = call(rows_of(pq, s * M, (s + 1) * M), rows_of(pk, ks_ * N, (ks_ + 1) * N), vt_of(ks_), 1, ql[s:s + 1].contiguous(),
                           kl[ks_:ks_ + 1].contiguous(), 0)
                stag = ops.last_kernel()
                ops.attention_split = c.get("split", True)
                rep.shared(out[s * M:s * M + qlens[s]], one[:qlens[s]], stag, ref, promise=True)
    rep.done(err)


RUNNERS = {"linear": run_linear, "linear_planes": run_linear_planes, "linear_qkv_planes": run_linear_qkv_planes, "mlp_tail": run_mlp_tail,
           "bgemm_nt": run_bgemm_nt, "bgemm_nt_planes": run_bgemm_nt_planes, "conv": run_conv, "attention_x3": run_attention,
           "attention_h16t": run_attention}


@pytest.mark.parametrize("case", TI.CASES, ids=TI.case_id)
def test_instantiation(dev, case):
    RUNNERS[case["entry"]](dev, case, Report(case))
    torch.cuda.synchronize()
