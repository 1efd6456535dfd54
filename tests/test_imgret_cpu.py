"""CPU: the numpy restatement of the image-retrieval stages (tests/imgret_ref.py) against straightforward numpy, the sampler, the
symbol surface, the Python module's defaults and refusals, and the margins of every discrete assertion tests/test_gpu_imgret.py
makes on a scene: an input whose margin is too thin is replaced here, not excused on the device."""
import inspect
from pathlib import Path

import numpy as np
import pytest

from tests import imgret_ref as IR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_imgret_assign", "pram_imgret_aggregate", "pram_imgret_fold", "pram_imgret_update", "pram_imgret_normalize",
           "pram_imgret_topk_workspace_bytes", "pram_imgret_topk")
# A discrete assertion on similarities holds on the device when the restatement's gap exceeds twice the bound of the fp32 chain
# against the float64 product (the vectors themselves are the same bits on both sides); required here: four times.
MARGIN = 4.0


# ---------------------------------------------------------------- the restatement against straightforward numpy
def test_assign_against_argmin():
    for n, k in ((65, 16), (257, 64)):
        x, c = IR.assign_case(n, k)
        lab, dist = IR.assign(x, c)
        d = ((x.astype(np.float64)[:, None, :] - c.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        assert np.allclose(dist, d.min(1), rtol=1e-13, atol=0)
        # argmin up to the planted duplicates, which the restatement gives to the lower index
        twin = {k - 1: 0, 7: 3}
        plain = np.array([twin.get(int(l), int(l)) for l in np.argmin(d, 1)])
        assert np.array_equal(lab, plain)
        assert not np.isin(lab, list(twin)).any()


def test_assign_margins():
    """The labels the GPU file asserts are exact because the distances are the same bits; what could still go wrong is a near tie
    decided by the order of a sum, and there is none: the runner-up is either an exact tie (a planted duplicate) or far."""
    ties = 0
    for n in IR.ASSIGN_ROWS:
        for k in IR.ASSIGN_K:
            if k == 1:
                continue
            x, c = IR.assign_case(n, k)
            s = np.sort(IR.dist2(x, c), 1)
            gap = (s[:, 1] - s[:, 0]) / s[:, 0]
            ties += int((gap == 0).sum())
            assert ((gap == 0) | (gap > 1e-9)).all(), (n, k, gap[gap > 0].min())
    assert ties > 100      # the tie rule is exercised


def test_vlad_against_plain_numpy():
    c, (x, first, cnt), batch, counts = IR.aggregate_case()
    lab, _ = IR.assign(x, c)
    sums, n = IR.aggregate(x, lab, c, first, cnt)
    out = IR.normalize(sums)
    for i, (a, m) in enumerate(zip(first, cnt)):
        rows, l = x[a:a + m].astype(np.float64), lab[a:a + m]
        V = np.stack([(rows[l == j] - c[j].astype(np.float64)).sum(0) if (l == j).any() else np.zeros(IR.DIM) for j in range(IR.AGG_K)])
        assert np.allclose(sums[i], V, rtol=1e-12, atol=1e-12) and np.array_equal(n[i], np.bincount(l, minlength=IR.AGG_K))
        nrm = np.linalg.norm(V, axis=1, keepdims=True)
        W = np.divide(V, nrm, out=np.zeros_like(V), where=nrm > 0).ravel()
        want = W / np.linalg.norm(W) if m else np.zeros_like(W)
        assert np.abs(out[i] - want).max() < 1e-7
    assert not out[0].any() and (n[1].sum() == 1) and (n[1] == 0).sum() == IR.AGG_K - 1      # no rows; centres nobody chooses
    assert abs(np.linalg.norm(out[2].astype(np.float64)) - 1.0) < 1e-6
    # the padded layout equals the flat layout of its real rows, and the NaN behind the counts never shows
    ps, pn, pout = IR.padded_vlad(batch, counts, c)
    assert np.isfinite(ps).all() and np.isfinite(pout).all() and not pout[0].any() and pn.sum(1).tolist() == list(IR.PADDED_COUNTS)


def test_topk_against_argsort():
    rng = np.random.RandomState(3)
    q, db = rng.standard_normal((7, 256)), rng.standard_normal((50, 256))
    S = q @ db.T
    idx, sim = IR.topk(S, 5)
    assert np.array_equal(idx, np.argsort(-S, 1, kind="stable")[:, :5]) and np.array_equal(sim, np.take_along_axis(S, idx.astype(np.int64), 1))
    idx, sim = IR.topk(S, 64, exclude=np.arange(7), db_valid=np.arange(50) % 2 == 0)
    assert (idx[:, 25:] == -1).all() and not sim[:, 25:].any() and (idx[:, :24] % 2 == 0).all()
    assert all(i not in idx[i] for i in range(7)) and (idx[1::2, 24] >= 0).all() and (idx[0::2, 24] == -1).all()
    # integer data: ties go to the lower index
    qi, di = IR.topk_int_case(33, 257, 128)
    Si = qi.astype(np.float64) @ di.astype(np.float64).T
    idx, sim = IR.topk(Si, 20)
    for i in range(33):
        key = list(zip((-sim[i]).tolist(), idx[i].tolist()))
        assert key == sorted(key)
    assert np.abs(Si).max() < 2 ** 24
    assert IR.unique_pairs([[1, 2], [0, 2], [0, -1]]) == [(0, 1), (0, 2), (1, 2)]


def test_sampler_picks():
    from pram_amd.localization import image_retrieval as M
    for n, k, seed in ((1025, 16, 5), (16, 16, 0), (300, 64, 2 ** 63 + 11), (1, 1, 3)):
        a = IR.initial_rows(n, k, seed)
        assert len(set(a.tolist())) == k and a.min() >= 0 and a.max() < n
        assert np.array_equal(a, IR.initial_rows(n, k, seed)) and np.array_equal(a, M.initial_rows(n, k, seed))
    assert not np.array_equal(IR.initial_rows(1025, 16, 5), IR.initial_rows(1025, 16, 6))
    assert sorted(IR.initial_rows(16, 16, 0).tolist()) == list(range(16))
    with pytest.raises(ValueError):
        M.initial_rows(5, 6, 0)


def test_vocabulary_restatement():
    x, picks = IR.vocab_case()
    c0 = x[picks]
    assert np.array_equal(c0[IR.VOCAB_STARVED], c0[IR.VOCAB_TWIN]) and IR.VOCAB_TWIN < IR.VOCAB_STARVED
    c1, n1 = IR.lloyd_step(x, c0)
    assert n1[IR.VOCAB_STARVED] == 0 and np.array_equal(c1[IR.VOCAB_STARVED], c0[IR.VOCAB_STARVED]) and n1.sum() == IR.VOCAB_N
    moved = [j for j in range(IR.VOCAB_K) if n1[j] > 0]
    lab, _ = IR.assign(x, c0)
    for j in moved[:3]:      # a moved centre is its rows' mean
        assert np.allclose(c1[j], x[lab == j].astype(np.float64).mean(0), atol=1e-5)
    assert np.array_equal(IR.train_vocabulary(x, IR.VOCAB_K, 1, IR.VOCAB_SEED), c1)


# ---------------------------------------------------------------- the symbol surface, defaults, refusals
def test_header_and_exports(hip_lib):
    from pram_amd import _lib, ops
    # exported == declared, by type, and header == ops for the PRAM_IMGRET_* constants: tests/test_abi_contract_cpu.py
    assert sorted(ENTRIES) == sorted(n for n in _lib.exported_symbols() if n.startswith("pram_imgret_"))
    assert IR.DIM == ops.IMGRET_DIM and IR.MAX_K == ops.IMGRET_MAX_K and IR.MAX_TOPK == ops.IMGRET_MAX_TOPK
    # the workspace function needs no device
    assert hip_lib.pram_imgret_topk_workspace_bytes(10, 20, 3) == 10 * 3 * 20 * 8
    assert hip_lib.pram_imgret_topk_workspace_bytes(10, 65, 1) == 0 and hip_lib.pram_imgret_topk_workspace_bytes(10, 0, 1) == 0
    assert hip_lib.pram_imgret_topk_workspace_bytes(10, 5, 0) == 0


def test_defaults_and_dispatch():
    from pram_amd._lib import PramHipError
    from pram_amd.localization import image_retrieval as M
    sig = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert sig(M.train_vocabulary) == dict(k=64, iters=20, seed=0, device="cuda")
    assert sig(M.global_descriptors) == dict(image_chunk=1024)
    assert sig(M.retrieve) == dict(exclude=None, db_valid=None, splits=None)
    assert M.VOCAB_BLOCK == IR.BLOCK
    x = np.zeros((4, 128), dtype=np.float32)
    with pytest.raises(TypeError):
        M.train_vocabulary(x, k=2, tol=1e-3)
    with pytest.raises(TypeError):
        M.retrieve(x, x, 2, metric="l2")
    with pytest.raises(TypeError):
        M.global_descriptors(None, [], chunk=3)
    with pytest.raises(TypeError):
        M.pairs_from_retrieval(x, 2, include_self=True)
    with pytest.raises(PramHipError):
        M.train_vocabulary(x, k=2, device="cpu")
    import torch
    with pytest.raises(PramHipError):
        M.retrieve(torch.zeros(2, 128), torch.zeros(3, 128), 2)
    with pytest.raises(PramHipError):
        M.Vocabulary(torch.zeros(4, 128))
    with pytest.raises(PramHipError):
        M.Vocabulary.load("nowhere.npz", device="cpu")
    assert M.default_splits(16, 10000) == 79 and M.default_splits(2000, 2000) == 9 and M.default_splits(1, 1) == 1 and M.default_splits(10 ** 6, 10 ** 6) == 1


# ---------------------------------------------------------------- the margins of the scenes' discrete assertions
def _gap_ok(gap: float, L: int) -> bool:
    return gap > MARGIN * IR.topk_eps(L)


def test_covisible_scene_margins():
    """What test_gpu_imgret.py asserts of refine_ref.covisible_scene, on the restatement, each with its gap."""
    c = IR.covisible()
    L = IR.COVIS_K * IR.DIM
    share, qs = c["share"], c["q_share"]
    vf, vq = c["v_frames"].astype(np.float64), c["v_queries"].astype(np.float64)
    F = len(vf)
    assert share[2, 0] == share[2, 1] == 40 and share[2].max() == 40      # either is right for frame 2
    S = vf @ vf.T
    for f in range(F):
        best = set(np.nonzero(share[f] == share[f].max())[0].tolist())
        rest = [g for g in range(F) if g != f and g not in best]
        gap = max(S[f, g] for g in best) - max(S[f, g] for g in rest)
        assert _gap_ok(gap, L), (f, gap)
    Sq = vq @ vf.T
    for b, want in enumerate(IR.COVIS_QUERY_TOP2):
        assert set(np.argsort(-qs[b], kind="stable")[:2].tolist()) == set(want)      # the two that share most pool points
        rest = [g for g in range(F) if g not in want]
        gap = min(Sq[b, g] for g in want) - max(Sq[b, g] for g in rest)
        assert _gap_ok(gap, L), (b, gap)
    assert qs[3].argmax() == 7 and _gap_ok(Sq[3, 7] - np.delete(Sq[3], 7).max(), L)
    assert c["queries"][4]["count"] == 0 and not vq[4].any()
    # the lists RetrievalIndex.query(features, 3) hands to the localizer: their cut is as clear
    for b in range(4):
        s = np.sort(Sq[b])[::-1]
        assert _gap_ok(s[2] - s[3], L), (b, s[:4])


def test_street_scene_margins():
    """The street scene: a frame shares points only with its neighbours, the restatement's lists cut clearly, every listed pair
    shares at least STREET_MIN_SHARE planted points (110 the fewest: frames 0 and 4), and every frame has neighbours enough."""
    st = IR.street()
    s, sh = st["scene"], st["scene"]["share"]
    F = s["n_frames"]
    assert F == IR.STREET_FRAMES and all(sh[a, b] == 0 for a in range(F) for b in range(F) if abs(a - b) > 6)
    assert all(sh[a, a + 1] > 400 for a in range(F - 1))
    L = IR.STREET_K * IR.DIM
    S = st["S"].copy()
    np.fill_diagonal(S, -np.inf)
    srt = -np.sort(-S, 1)
    assert all(_gap_ok(srt[f, IR.STREET_MATCHED - 1] - srt[f, IR.STREET_MATCHED], L) for f in range(F))
    assert min(sh[a, b] for a, b in st["pairs"]) >= IR.STREET_MIN_SHARE
    assert len(st["pairs"]) == len({frozenset(p) for p in st["pairs"]}) and all(a != b for a, b in st["pairs"])
    m = IR.street_matches(s, st["pairs"][:3] + [(4, 1)])
    assert np.array_equal(m[0], IR.street_matches(s, [st["pairs"][0]])[0])      # a pair's list does not depend on the request
    a, b = st["pairs"][0]
    inv = lambda f: {k: pt for (g, pt), k in s["where"].items() if g == f}
    ia, ib = inv(a), inv(b)
    right = sum(1 for i, j in m[0].tolist() if i in ia and ia[i] == ib.get(j, -2))
    assert abs(right / len(m[0]) - 0.8) < 0.02 and abs(right - 0.9 * sh[a, b]) < 0.05 * sh[a, b]      # a fifth wrong
    rev = IR.street_matches(s, [(1, 4)])[0]
    assert np.array_equal(m[3], rev[:, ::-1])
