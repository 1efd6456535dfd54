"""GPU: the small integer-valued kernels between the models, each called directly and compared with its plain restatement
(tests/glue_ref.py): row top-2, projection top-2 (float32 and float64 projections), projection and compaction of map points,
the recogniser epilogue, the full row sort, the landmark vote, AdaGML pruning / layer state / scatter / score packing, descriptor
sampling, score lookup, row normalisation and bilinear resize.  Everything that is an index, a count or a copy must be equal;
floating-point outputs are held to the bars the suite already applies to the same quantities.  tests/test_glue_ref_cpu.py
checks, without a GPU, that the seeded inputs meet the conditions under which these comparisons are exact."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import glue_ref as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _i32(v, dev):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=dev)


def _np(t):
    return t.cpu().numpy()


def _diff(got, want) -> float:
    """largest |got - want| over the finite entries of the float64 yardstick; the others (+-inf) must be equal"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), (got[~fin], want[~fin])
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


# ------------------------------------------------------------------------------------------------ row top-2
@pytest.mark.parametrize("largest", [True, False])
def test_row_top2(dev, largest):
    """Values are copies of the input and must be bit-equal, the index exact, ties to the lowest index; garbage beyond n_valid is
    never read; at n = 1 the second value is -inf / +inf."""
    from pram_amd import ops
    for M in G.TOP2_M:
        for n in G.TOP2_N:
            c = G.top2_case(M, n, largest)
            v0, v1, i0 = ops.row_top2(c["x"].to(dev), largest, n_valid=n)
            w0, w1, wi = G.row_top2(c["x"], largest, n_valid=n)
            assert np.array_equal(_np(i0), wi), (M, n)
            assert np.array_equal(_np(v0), w0.astype(np.float32)) and np.array_equal(_np(v1), w1.astype(np.float32)), (M, n)
            if n == 1:
                assert np.all(_np(v1) == (-np.inf if largest else np.inf))
            for b, r in c["ties"]:
                if n > 1:
                    assert float(v1[b, r]) == float(v0[b, r])
            if M == 5 and n == 70:
                assert _np(i0)[0, :4].tolist() == [3, 5, 4, 0] and float(v1[0, 2]) == (1.5 if largest else -1.5)
    c = G.top2_case(5, 70, largest)
    for row_lens, col_lens in G.TOP2_RAGGED:
        v0, v1, i0 = ops.row_top2(c["x"].to(dev), largest, row_lens=_i32(row_lens, dev), col_lens=_i32(col_lens, dev))
        w0, w1, wi = G.row_top2(c["x"], largest, row_lens=row_lens, col_lens=col_lens)
        assert np.array_equal(_np(i0), wi), (row_lens, col_lens)
        assert np.array_equal(_np(v0), w0.astype(np.float32)) and np.array_equal(_np(v1), w1.astype(np.float32))
        for b in range(G.TOP2_B):
            assert np.all(_np(i0)[b, row_lens[b]:] == -1) and np.all(_np(v0)[b, row_lens[b]:] == 0) and np.all(_np(v1)[b, row_lens[b]:] == 0)
            if col_lens[b] == 0:
                assert row_lens[b] > 0 and np.all(_np(i0)[b, :row_lens[b]] == -1)
    print(f"row_top2 largest={largest}: values and indices equal")


# ------------------------------------------------------------------------------------------------ projection top-2
@pytest.mark.parametrize("f64uv", [False, True])
def test_proj_dist_top2(dev, f64uv):
    from pram_amd import ops
    worst = 0.0
    for M in G.PROJ_M:
        for n in G.PROJ_N:
            c = G.proj_case(M, n)
            if f64uv:
                d0, d1, i0 = ops.proj_dist_top2_f64uv(c["sim"].to(dev), c["kpts"].to(dev), c["uv64"].to(dev), G.PROJ_RANGE, n)
            else:
                d0, d1, i0 = ops.proj_dist_top2(c["sim"].to(dev), c["kpts"].to(dev), c["uv"].to(dev), G.PROJ_RANGE, n_valid=n)
            w0, w1, wi = G.proj_dist_top2(c["sim"], c["kpts"], c["uv"], G.PROJ_RANGE, n)
            assert np.array_equal(_np(i0), wi), (M, n, _np(i0), wi)
            worst = max(worst, _diff(_np(d0), w0), _diff(_np(d1), w1))
            for r in c["ties"]:
                assert float(d0[r]) == float(d1[r]) and float(d0[r]) < 1.0
            if M == 6:
                assert float(d0[2]) >= 100.0                                      # every column penalised
                if c["exact_col"] is not None:                                    # pixel distance == range: penalised
                    col = c["exact_col"]
                    assert G.proj_dist(c["sim"], c["kpts"], c["uv"], G.PROJ_RANGE, n)[3, col] >= 100.0
                    assert (int(i0[3]) != col) if n > 1 else float(d0[3]) >= 100.0
    print(f"proj_dist_top2 f64uv={f64uv}: max |d - fp64| = {worst:.3e} (bar 1e-4)")
    assert worst < 1e-4


# ------------------------------------------------------------------------------------------------ projection of the map points
def _check_projection(dev, c):
    from pram_amd import ops
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64).to(dev)
    uvd, mask, keep, uvk, count = ops.project_points(f(c["xyz"]).reshape(-1, 3), f(c["K"]), f(c["T"]), c["w"], c["h"])
    wu, wm, wk = G.project_points(c["xyz"], c["K"], c["T"], c["w"], c["h"])
    n = int(count.item())
    assert np.array_equal(_np(mask) != 0, wm)
    assert n == len(wk) and np.array_equal(_np(keep)[:n], wk)
    assert torch.equal(uvk[:, :n], uvd[:2, keep[:n].long()])
    return _diff(_np(uvd), wu), wm


def test_project_points(dev):
    worst = 0.0
    for n in G.PP_N:
        d, m = _check_projection(dev, G.pp_case(n))
        worst = max(worst, d)
    d, m = _check_projection(dev, G.pp_case(1500, "inside"))
    assert m.all()
    worst = max(worst, d)
    d, m = _check_projection(dev, G.pp_case(1500, "outside"))
    assert not m.any()
    worst = max(worst, d)
    c = G.pp_boundary_case()
    d, m = _check_projection(dev, c)
    assert np.array_equal(m, c["expect"])
    worst = max(worst, d)
    print(f"project_points: max |uvd - fp64| = {worst:.3e} (bar 1e-9)")
    assert worst < 1e-9


# ------------------------------------------------------------------------------------------------ recogniser epilogue
@pytest.mark.parametrize("C", G.SEG_C)
def test_seg_epilogue(dev, C):
    from pram_amd import ops
    worst = 0.0
    for N in G.SEG_N:
        c = G.seg_case(N, C)
        for lens in (None, c["lens"]):
            for thr in (G.SEG_THR, 2.0):
                wi, wm, wc, ws = G.seg_epilogue(c["x"], lens, thr)
                for want_scores in (True, False):
                    ids, mask, cnt, sc = ops.seg_epilogue(c["x"].to(dev), _i32(lens, dev), thr, want_scores=want_scores)
                    assert np.array_equal(_np(ids), wi) and np.array_equal(_np(mask), wm), (N, C, lens, thr)
                    assert np.array_equal(_np(cnt), wc) and np.array_equal(_np(cnt), _np(mask).sum(1))
                    assert (sc is not None) == want_scores
                    if want_scores:
                        worst = max(worst, _diff(_np(sc), ws))
                        if lens is not None:
                            for b in range(G.SEG_B):
                                assert not _np(sc)[b, lens[b]:].any()
                assert wi[0, 0] == c["tie"][0] - 1                                      # the tie: first occurrence
                if N >= 3 and thr < 1:
                    assert wm[0, 1] == 0 and wm[0, 2] == 1
                if thr == 2.0:                                                          # keeps every token there is
                    assert wm.sum() == (sum(lens) if lens is not None else G.SEG_B * N)
    print(f"seg_epilogue C={C}: max |softmax - fp64| = {worst:.3e} (bar 1e-6)")
    assert worst < 1e-6


# ------------------------------------------------------------------------------------------------ full row sort
def _check_sort(dev, x):
    from pram_amd import ops
    v, i = ops.row_sort_desc(x.to(dev))
    o = torch.sort(x, dim=-1, descending=True, stable=True)
    assert torch.equal(i.cpu(), o.indices)
    assert torch.equal(v.cpu(), o.values)
    assert torch.equal(v.cpu().view(torch.int32), torch.gather(x, 1, o.indices).view(torch.int32))      # the input's own bits


@pytest.mark.parametrize("cols", G.SORT_COLS)
def test_row_sort_desc(dev, cols):
    _check_sort(dev, G.sort_case(cols))


def test_row_sort_desc_zeros_and_limit(dev):
    """+0.0 and -0.0 are equal: they keep their index order (torch.sort, stable) and their own sign bits; 1025 columns are refused."""
    from pram_amd import ops
    from pram_amd._lib import PramHipError
    _check_sort(dev, G.sort_zero_case())
    with pytest.raises(PramHipError):
        ops.row_sort_desc(torch.zeros(2, 1025, device=dev))


# ------------------------------------------------------------------------------------------------ landmark vote
def _check_vote(got, want, n, topk):
    sid, rank, cnt, nwin, tokens, mean = (_np(t) for t in got)
    assert int(nwin.reshape(-1)[0]) == len(want) <= topk
    worst = 0.0
    for w, (s, k, tok, m) in enumerate(want):
        assert (sid[w], rank[w], cnt[w]) == (s, k, len(tok)), (w, sid[w], rank[w], cnt[w], s, k, len(tok))
        assert np.array_equal(tokens[w, :len(tok)], tok)
        worst = max(worst, abs(float(mean[w]) - m))
    return worst


@pytest.mark.parametrize("n,C,topk", G.VOTE_CASES)
def test_seg_vote(dev, n, C, topk):
    from pram_amd import ops
    c = G.vote_case(n, C, topk)
    want = G.seg_vote(c["ids"], c["vals"], topk)
    worst = _check_vote(ops.seg_vote(c["vals"].to(dev), c["ids"].to(dev), topk), want, n, topk)
    if n:       # second opinion: the oracle's host loop on the score matrix that sorts into these lists
        ps = R.process_segmentations(torch.from_numpy(G.vote_segs(c)), topk=topk)
        assert [int(p[0]) for p in ps] == [w[0] for w in want] and all(np.array_equal(np.asarray(p[1]), w[2]) for p, w in zip(ps, want))
    print(f"seg_vote {(n, C, topk)}: {len(want)} winners, max |mean - fp64| = {worst:.3e} (bar 1e-6)")
    assert worst < 1e-6


def test_seg_vote_batched(dev):
    from pram_amd import ops
    n, C, topk = 70, 9, 3
    cases = [G.vote_case(n, C, topk, v) for v in range(3)]
    ids, vals = torch.stack([c["ids"] for c in cases]).to(dev), torch.stack([c["vals"] for c in cases]).to(dev)
    got = ops.seg_vote_batched(vals, ids, topk)
    worst = 0.0
    for b, c in enumerate(cases):
        one = ops.seg_vote(vals[b].contiguous(), ids[b].contiguous(), topk)
        for g, o in zip(got, one):
            assert torch.equal(g[b].reshape(-1), o.reshape(-1))
        worst = max(worst, _check_vote([g[b] for g in got], G.seg_vote(c["ids"], c["vals"], topk), n, topk))
    assert worst < 1e-6
    empty = ops.seg_vote_batched(torch.zeros(3, 0, 5, device=dev), torch.zeros(3, 0, 5, device=dev, dtype=torch.int64), 3)
    assert _np(empty[3]).tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ AdaGML pruning
@pytest.fixture(scope="module")
def prune_states(dev):
    return {T: {k: (v, v.to(dev)) for k, v in G.prune_state(T).items()} for T in G.PRUNE_T}


@pytest.mark.parametrize("T", G.PRUNE_T)
def test_adagml_prune(dev, prune_states, T):
    from pram_amd import ops
    st = prune_states[T]
    lens = G.prune_lens(T)
    worst = 0.0
    for kind in G.PRUNE_KINDS:
        lg, thr = G.prune_logits(T, kind)
        keep, below, wconf = G.adagml_prune(lg, thr, G.PRUNE_NMIN, lens, T)
        assert len(keep[2]) == 7 and len(keep[3]) == 0                       # below n_min_tokens: kept whole
        if kind == "all":
            assert [len(k) for k in keep] == lens and not below.any()
        if kind == "none":
            assert [len(k) for k in keep] == [0, 0, 7, 0] and below.tolist() == lens
        if kind == "last":
            assert keep[0].tolist() == [T - 3, T - 2, T - 1] and keep[1].tolist() == [T - 4, T - 3, T - 2]
        for ld_logit in (1, 4):
            logit = (lg if ld_logit == 1 else G.prune_logits4(lg)).to(dev)
            for want_conf in (True, False):
                xo, co, so, io, lo, nb, conf = ops.adagml_prune(logit, thr, G.PRUNE_NMIN, _i32(lens, dev), st["x"][1], st["cos"][1], st["sin"][1],
                                                                st["ind"][1], want_conf=want_conf, ld_logit=ld_logit)
                assert _np(lo).tolist() == [len(k) for k in keep], (kind, ld_logit, _np(lo), [len(k) for k in keep])
                assert np.array_equal(_np(nb), below), (kind, ld_logit)
                for s, k in enumerate(keep):
                    k = torch.from_numpy(k)
                    for name, o in (("x", xo), ("cos", co), ("sin", so), ("ind", io)):
                        assert torch.equal(o[s, :len(k)].cpu(), st[name][0][s, k]), (kind, ld_logit, s, name)
                assert (conf is not None) == want_conf
                if want_conf:
                    worst = max(worst, _diff(_np(conf), wconf))
                    for s, n in enumerate(lens):
                        assert not _np(conf)[s, n:].any()
    print(f"adagml_prune T={T}: max |conf - fp64 sigmoid| = {worst:.3e} (bar 1e-6)")
    assert worst < 1e-6


def test_adagml_prune_refuses_long_sets(dev):
    from pram_amd import ops
    from pram_amd._lib import PramHipError
    T = 8193
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
    with pytest.raises(PramHipError):
        ops.adagml_prune(z(1, T), 0.5, 8, None, z(1, T, 4), z(1, T, 32), z(1, T, 32), z(1, T, dt=torch.int32))


def test_adagml_scores4(dev):
    from pram_amd import ops
    from pram_amd import weights as W
    for shape in ((3, 70), (1, 1)):
        a, b = W.uniform(11, "s4/a", shape), W.uniform(11, "s4/b", shape)
        out = ops.adagml_scores4(a.to(dev), b.to(dev)).cpu()
        want = G.adagml_scores4(a, b)
        assert tuple(out.shape) == (a.numel(), 4) and torch.equal(out, want)


def test_adagml_layer_state(dev):
    """The kernel and the restated per-pair loop, side by side through a first, a middle and a last layer."""
    from pram_amd import ops
    B, T = G.LS_B, G.LS_T
    states = {None: G.layer_state_init()}
    for name, lens_new, n_below, ind_seed, layer, last, prev in G.layer_state_steps():
        st = states[prev]
        ind = G.layer_state_ind(ind_seed)
        want = G.adagml_layer_state(st, lens_new, n_below, ind, layer, last)
        d = {k: torch.from_numpy(np.array(st[k], copy=True)).to(dev) for k in ("active", "lens", "tiny", "stop_layer", "lens_final", "ind_final", "num_points")}
        a, l, lstop, leff = ops.adagml_layer_state(d["active"], d["lens"], _i32(lens_new, dev), _i32(n_below, dev), d["num_points"], d["tiny"],
                                                   d["stop_layer"], d["lens_final"], torch.from_numpy(ind).to(dev), d["ind_final"], B, T, layer, last)
        got = {"active": a, "lens": l, "lens_stop": lstop, "lens_eff": leff, "tiny": d["tiny"], "stop_layer": d["stop_layer"],
               "lens_final": d["lens_final"], "ind_final": d["ind_final"]}
        for k, v in got.items():
            assert np.array_equal(_np(v), want[k]), (name, k, _np(v), want[k])
        for s in range(2 * B):      # only the pairs that stop here commit their survivor ids
            stops = bool(st["active"][s % B]) and not want["active"][s % B]
            assert np.array_equal(_np(d["ind_final"])[s], ind[s] if stops else st["ind_final"][s]), (name, s)
        states[name] = {k: want[k] for k in st}
    assert states["first"]["active"].tolist() == [1, 1, 0] and states["middle"]["active"].tolist() == [0, 1, 0]
    assert states["middle"]["tiny"].tolist() == [0, 1, 0] and states["middle"]["stop_layer"].tolist() == [3, -1, 1]
    assert states["last"]["active"].tolist() == [0, 0, 0] and states["last"]["lens_final"].tolist() == [30, 4, 35, 29, 20, 33]
    assert states["last_unpruned"]["lens_final"].tolist() == [30, 5, 35, 29, 30, 33]


def test_adagml_scatter(dev):
    from pram_amd import ops
    c = G.scatter_case()
    for lens0 in (c["lens0"], None):
        om, osc = ops.adagml_scatter(c["m0"].to(dev), c["ms0"].to(dev), c["ind0"].to(dev), c["ind1"].to(dev), _i32(lens0, dev), c["m_full"])
        wm, ws = G.adagml_scatter(c["m0"], c["ms0"], c["ind0"], c["ind1"], lens0, c["m_full"])
        assert np.array_equal(_np(om), wm) and np.array_equal(_np(osc), ws)
        assert (wm == -1).sum() > c["m_full"] and (c["m0"] == -1).any()


# ------------------------------------------------------------------------------------------------ sampling tail
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("C", G.SAMPLE_C)
def test_sample_nhwc(dev, C, ragged):
    from pram_amd import ops
    fmap = G.sample_fmap(C)
    lens = [G.SAMPLE_N, 3] if ragged else None
    worst = 0.0
    for s, norms in ((4, (True, False)), (0, (False,))):
        kp = G.sample_kpts(s)
        for l2 in norms:
            out = ops.sample_nhwc(fmap.to(dev), kp.to(dev), _i32(lens, dev), s, l2)
            want = G.sample_nhwc(fmap, kp, lens, s, l2)
            worst = max(worst, _diff(_np(out), want.numpy()))
            if ragged:
                assert not _np(out)[1, 3:].any()
    print(f"sample_nhwc C={C} ragged={ragged}: max |sample - fp64| = {worst:.3e} (bar 2e-6)")
    assert worst < 2e-6


@pytest.mark.parametrize("C", G.SAMPLE_C)
def test_sample_nhwc_leaves_rows_beyond_lens_alone(dev, hip_lib, C):
    """The entry called on an output prefilled with a sentinel: rows at and beyond lens[b] keep it bit for bit (a store that runs
    past its own row lands in the next one: at C = 256 and 260 the second float4 of a lane ends exactly at the row's end), the
    rows before equal the wrapper's."""
    from pram_amd import ops
    fmap, kp = G.sample_fmap(C).to(dev), G.sample_kpts(4).to(dev)
    lens = [G.SAMPLE_N - 1, 3]
    B, fh, fw, _ = fmap.shape
    for l2 in (0, 1):
        out = torch.full((B, G.SAMPLE_N, C), 7.0, device=dev)
        rc = hip_lib.pram_sample_nhwc_f32(fmap.data_ptr(), B, fh, fw, C, kp.data_ptr(), _i32(lens, dev).data_ptr(), G.SAMPLE_N, 4, l2,
                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        ref = ops.sample_nhwc(fmap, kp, None, 4, bool(l2))
        for b in range(B):
            assert torch.equal(out[b, :lens[b]], ref[b, :lens[b]]) and bool((out[b, lens[b]:] == 7.0).all()), (C, l2, b)


def test_score_lookup(dev):
    from pram_amd import ops
    c = G.lookup_case()
    for maps in (c["maps"], c["maps"][:1]):                 # one map per set (stride path), one map for both sets
        for lens in (None, c["lens"]):
            out = ops.score_lookup(maps.to(dev), c["kpts"].to(dev), _i32(lens, dev))
            assert torch.equal(out.cpu(), G.score_lookup(maps, c["kpts"], lens))


def test_l2norm_rows(dev):
    from pram_amd import ops
    worst = 0.0
    for rows in G.L2_ROWS:
        for cols in G.L2_COLS:
            x = G.l2norm_case(rows, cols)
            out = ops.l2norm_rows_(x.clone().to(dev))
            worst = max(worst, _diff(_np(out), G.l2norm_rows(x).numpy()))
            if rows > 1:
                assert not _np(out)[1].any()
    print(f"l2norm_rows_: max |x / ||x|| - fp64| = {worst:.3e} (bar 1e-6)")
    assert worst < 1e-6


@pytest.mark.parametrize("src,dst", G.RESIZE_CASES)
def test_resize_bilinear(dev, src, dst):
    from pram_amd import ops
    x = G.resize_case(*src)
    out = ops.resize_bilinear(x.to(dev), *dst).cpu()
    d = _diff(out.numpy(), G.resize_bilinear(x[None], *dst)[0].numpy())
    print(f"resize_bilinear {src} -> {dst}: max |out - fp64| = {d:.3e} (bar 1e-6)")
    assert d < 1e-6
    if src == dst:
        assert torch.equal(out, x)
