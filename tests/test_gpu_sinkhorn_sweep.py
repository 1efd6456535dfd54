"""GPU (MI355X): pram_amd/csrc/sinkhorn.hip swept over every shape class of its kernel family, against the oracle in fp64.

Two kinds of assertion, neither leaving anything out:
  1. plan accuracy: ``p`` (want_p=True) against oracle/ref_cpu.py run in float64, at the bars the suite already uses against
     the fp32 goldens (Sinkhorn |p - ref| - 2e-6 |ref| < 1e-6, dual softmax |p - ref| < 1e-5).  tests/test_sinkhorn_inputs_cpu.py
     proves on the CPU that the fp32 oracle itself meets both bars on these exact inputs, so the bars are conditions the inputs
     satisfy, not allowances.  The largest device deviation of every case is printed (profiles/sinkhorn_parity.md records them).
  2. match extraction, exact: matches0/1 and matching_scores0/1 equal R.compute_matches applied on the host to the DEVICE's
     own ``p``, bit for bit, every row and column, lowest-index tie rule included; and the want_p=False instantiation returns
     the same four outputs bit for bit.  (The fp64 oracle's matches are not compared: top-2 gaps of these plans go down to
     ~5e-6 relative.)
The inputs, shape classes and bars live in tests/sinkhorn_cases.py."""
import pytest
import torch

from oracle import ref_cpu as R
from tests import sinkhorn_cases as S

pytestmark = pytest.mark.gpu

OUT4 = ("matches0", "matches1", "matching_scores0", "matching_scores1")


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-equal (floats compared as their 32-bit patterns)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _call(dev, M, bin_score, iters, thr, dual, want_p=True, lens=None, **kw):
    from pram_amd import ops
    if lens is not None:
        kw["m_lens"] = torch.tensor([l[0] for l in lens], dtype=torch.int32, device=dev)
        kw["n_lens"] = torch.tensor([l[1] for l in lens], dtype=torch.int32, device=dev)
    r = ops.sinkhorn_match(M.to(dev).contiguous(), torch.tensor(bin_score, device=dev), iters, thr, want_p=want_p,
                           dual_softmax=dual, **kw)
    return {k: v.cpu() for k, v in r.items()}


def _assert_matches_of_own_plan(out, p, thr, what):
    """The four discrete outputs == compute_matches of the device's own plan, bit for bit."""
    exp = dict(zip(OUT4, R.compute_matches(p, thr)))
    for k in OUT4:
        assert _same(out[k], exp[k]), (what, thr, k, int((out[k] != exp[k]).sum()))


def plan_deviation(dev, c: S.Case, dual: bool):
    """-> (input, device outputs for threshold 0, deviation figure against the fp64 oracle, (max abs, max relative) error)."""
    M = S.case_input(c)
    out = _call(dev, M, c.bin, c.iters, 0.0, dual)
    ref = S.reference(M, c.bin, c.iters, dual)
    return M, out, S.deviation(out["p"], ref, dual), S.abs_rel(out["p"], ref)


SWEEP = [(c, False) for c in S.CASES] + [(c, True) for c in S.CASES if c.kind != "iter"]      # the dual path has no iterations


@pytest.mark.parametrize("c,dual", SWEEP, ids=[f"{'dual' if d else 'sinkhorn'}-{c.id}" for c, d in SWEEP])
def test_sweep(dev, c, dual):
    M, out0, d, (ea, er) = plan_deviation(dev, c, dual)
    print(f"\n{'dual' if dual else 'sinkhorn'} NV={c.nv} {c.id}: device deviation {d:.3e} (bar {S.bar(dual):g}) abs {ea:.3e} rel {er:.3e}")
    assert tuple(out0["p"].shape) == (S.BATCH, c.m + 1, c.n + 1) and bool(torch.isfinite(out0["p"]).all())
    assert d < S.bar(dual), d
    p = out0["p"]
    for rA, rB, cA, cB in c.ties:      # the planted ties are exact ties of the device's plan, and they are the maxima
        inner = p[:, :-1, :-1]
        top = inner[:, rA, cA]
        for r_, c_ in ((rA, cB), (rB, cA), (rB, cB)):
            assert _same(inner[:, r_, c_], top), (r_, c_)
        assert _same(inner[:, rA].max(1).values, top) and _same(inner[:, :, cA].max(1).values, top)
    for thr in S.THRESHOLDS:
        out = out0 if thr == 0.0 else _call(dev, M, c.bin, c.iters, thr, dual)
        assert _same(out["p"], p)
        _assert_matches_of_own_plan(out, p, thr, "want_p=True")
        lean = _call(dev, M, c.bin, c.iters, thr, dual, want_p=False)
        assert "p" not in lean
        for k in OUT4:
            assert _same(lean[k], out[k]), ("want_p=False", thr, k)
    for rA, rB, cA, cB in c.ties:      # lowest index wins both ways; the copies stay unmatched
        assert out0["matches0"][:, rA].tolist() == [cA] * S.BATCH and out0["matches1"][:, cA].tolist() == [rA] * S.BATCH
        assert out0["matches0"][:, rB].tolist() == [-1] * S.BATCH and out0["matches1"][:, cB].tolist() == [-1] * S.BATCH


# ---- ragged batches --------------------------------------------------------------------------------------------------
def _assert_ragged(outs, M, lens, bin_score, dual, what):
    """outs: {threshold: outputs}.  Inside the lengths: plan against the fp64 oracle on the unpadded sub-matrix, matches of the
    device's own sub-plan.  Outside: exactly 0 (plan, scores) and exactly -1 (matches)."""
    worst = -1.0
    for b, (m, n) in enumerate(lens):
        for thr, out in outs.items():
            p = out["p"][b]
            sub = p[:m + 1, :n + 1]
            if thr == 0.0:
                d = S.deviation(sub[None], S.reference(M[b:b + 1, :m, :n], bin_score, 20, dual), dual)
                worst = max(worst, d)
                assert d < S.bar(dual), (what, b, m, n, d)
            outside = p.clone()
            outside[:m + 1, :n + 1] = 0
            assert bool((outside == 0).all()), (what, b, "plan padding")
            if m > 0 and n > 0:
                exp = dict(zip(OUT4, R.compute_matches(sub[None], thr)))
            else:      # an element with an empty side reports no matches
                exp = {"matches0": torch.full((1, m), -1), "matches1": torch.full((1, n), -1),
                       "matching_scores0": torch.zeros(1, m), "matching_scores1": torch.zeros(1, n)}
            for k, length in zip(OUT4, (m, n, m, n)):
                assert _same(out[k][b, :length], exp[k][0]), (what, b, thr, k)
                pad = out[k][b, length:]
                assert bool((pad == (-1 if k.startswith("matches") else 0)).all()), (what, b, thr, k, "padding")
    return worst


def _poisoned(M, lens, value):
    Mp = M.clone()
    for b, (m, n) in enumerate(lens):
        Mp[b, m:, :] = value
        Mp[b, :, n:] = value
    return Mp


@pytest.mark.parametrize("dual", [False, True], ids=["sinkhorn", "dual"])
@pytest.mark.parametrize("m_max,n_max", S.RAGGED_SHAPES)
def test_ragged(dev, m_max, n_max, dual):
    M, lens, bs = S.ragged_input(m_max, n_max), S.ragged_lens(m_max, n_max), S.RAGGED_BIN[n_max]
    outs = {thr: _call(dev, M, bs, 20, thr, dual, lens=lens) for thr in S.THRESHOLDS}
    worst = _assert_ragged(outs, M, lens, bs, dual, "ragged")
    print(f"\n{'dual' if dual else 'sinkhorn'} NV={S.nv_of(n_max)} ragged {m_max}x{n_max}: device deviation {worst:.3e}")
    base = outs[0.2]
    lean = _call(dev, M, bs, 20, 0.2, dual, want_p=False, lens=lens)
    for k in OUT4:
        assert _same(lean[k], base[k]), ("want_p=False", k)
    # the padding of dist is never read into a result
    for poison in (float("nan"), 1e30):
        got = _call(dev, _poisoned(M, lens, poison), bs, 20, 0.2, dual, lens=lens)
        for k in OUT4 + ("p",):
            assert _same(got[k], base[k]), ("poisoned padding", poison, k)
        # n_valid < ldd: columns padded to the next multiple of 4 with the same poison
        ldd = (n_max + 3) // 4 * 4
        assert ldd > n_max
        wide = torch.cat([_poisoned(M, lens, poison), torch.full((M.shape[0], m_max, ldd - n_max), poison)], -1)
        got = _call(dev, wide, bs, 20, 0.2, dual, lens=lens, n_valid=n_max)
        for k in OUT4 + ("p",):
            assert _same(got[k], base[k]), ("n_valid < ldd", poison, k)


# ---- grouping --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dual", [False, True], ids=["sinkhorn", "dual"])
def test_grouped_call_equals_one_call(dev, hip_lib, monkeypatch, dual):
    """ops.sinkhorn_match slices dist, m_lens, n_lens, p and the four outputs per group: B = 9 ragged pairs as groups of 4, 4
    and 1 return every output bit-equal to the run with grouping off."""
    from pram_amd import ops
    M, lens = S.group_input(), S.GROUP_LENS
    m_max, n_max = S.GROUP_SHAPE
    sizes = []
    real = hip_lib.pram_sinkhorn_workspace_bytes

    def spy(nb, m, n):
        sizes.append(nb)
        return real(nb, m, n)

    monkeypatch.setattr(hip_lib, "pram_sinkhorn_workspace_bytes", spy)
    monkeypatch.setattr(ops, "sinkhorn_group_bytes", 0)
    whole = {thr: _call(dev, M, 1.0, 20, thr, dual, lens=lens) for thr in S.THRESHOLDS}
    assert sizes == [9, 9]
    _assert_ragged(whole, M, lens, 1.0, dual, "ungrouped")
    per_pair = (m_max + 1) * ((n_max + 4) // 4 * 4) * 4
    monkeypatch.setattr(ops, "sinkhorn_group_bytes", 4 * per_pair + per_pair // 2)
    del sizes[:]
    for thr in S.THRESHOLDS:
        grouped = _call(dev, M, 1.0, 20, thr, dual, lens=lens)
        for k in OUT4 + ("p",):
            assert _same(grouped[k], whole[thr][k]), (thr, k)
    assert sizes == [4, 4, 1, 4, 4, 1]


# ---- the C entry points, through ctypes ------------------------------------------------------------------------------
def _entry(lib, dual, dist, bs, m_max, n_max, ws, p=None, ldp=0, m0=None, m1=None, s0=None, s1=None):
    ptr = lambda t: None if t is None else t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    head = (ptr(dist), dist.shape[2], None, None, ptr(bs))
    tail = (ptr(p), ldp, ptr(m0), ptr(m1), ptr(s0), ptr(s1), dist.shape[0], m_max, n_max, ptr(ws), st)
    if dual:
        return lib.pram_dual_softmax_match_f32(*head, 0.2, *tail)
    return lib.pram_sinkhorn_match_f32(*head, 20, 0.2, *tail)


@pytest.mark.parametrize("dual", [False, True], ids=["sinkhorn", "dual"])
def test_c_entry_null_outputs_and_argument_errors(dev, hip_lib, dual):
    B, m, n = 2, 37, 150
    dist = S.sink_input("centry", B, m, n).to(dev)
    bs = torch.tensor([0.0], device=dev)
    ws = torch.empty(hip_lib.pram_sinkhorn_workspace_bytes(B, m, n), dtype=torch.uint8, device=dev)
    full = {"p": torch.zeros(B, m + 1, n + 1, device=dev), "m0": torch.empty(B, m, dtype=torch.int64, device=dev),
            "m1": torch.empty(B, n, dtype=torch.int64, device=dev), "s0": torch.empty(B, m, device=dev), "s1": torch.empty(B, n, device=dev)}
    assert _entry(hip_lib, dual, dist, bs, m, n, ws, ldp=n + 1, **full) == 0
    _assert_matches_of_own_plan({"matches0": full["m0"].cpu(), "matches1": full["m1"].cpu(), "matching_scores0": full["s0"].cpu(),
                                 "matching_scores1": full["s1"].cpu()}, full["p"].cpu(), 0.2, "C entry")
    m0, s0 = torch.full_like(full["m0"], -7), torch.full_like(full["s0"], -7.0)
    assert _entry(hip_lib, dual, dist, bs, m, n, ws, m0=m0, s0=s0) == 0      # p_out, matches1 and mscores1 null
    assert _same(m0.cpu(), full["m0"].cpu()) and _same(s0.cpu(), full["s0"].cpu())
    # argument errors: nothing is launched, nothing is written
    m0.fill_(-7)
    assert _entry(hip_lib, dual, dist, bs, m, n, ws, ldp=n, **full) == -1 and b"ldp" in hip_lib.pram_last_error()
    assert _entry(hip_lib, dual, dist, bs, m, S.N_LIMIT + 1, ws, m0=m0, s0=s0) == -1 and b"4351 columns" in hip_lib.pram_last_error()
    assert _entry(hip_lib, dual, dist, bs, S.M_LIMIT + 1, n, ws, m0=m0, s0=s0) == -1 and b"8191 rows" in hip_lib.pram_last_error()
    assert bool((m0 == -7).all())


@pytest.mark.parametrize("dual", [False, True], ids=["sinkhorn", "dual"])
def test_more_than_8191_rows_is_refused(dev, dual):
    """A wave keeps one row's result per lane: 32 blocks x 4 waves x 64 lanes = 8192 rows, the dust-bin row included.  One row
    more used to return a wrong plan with status 0 (m = 8191 itself is in the sweep above)."""
    from pram_amd import ops
    from pram_amd._lib import PramHipError
    with pytest.raises(PramHipError, match="8191 rows"):
        ops.sinkhorn_match(torch.zeros(1, S.M_LIMIT + 1, 8, device=dev), torch.tensor(1.0, device=dev), 20, 0.2, dual_softmax=dual)
