"""CPU: the numpy restatement of the two-view estimator (tests/twoview_ref.py) against planted geometry and scipy, the margins that
make the device's discrete results exact, the header and the exports, and the host logic of pram_amd.localization.twoview."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import pose_ref as PR
from tests import twoview_ref as TR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_twoview_hypotheses", "pram_twoview_score", "pram_twoview_finish")
SOLVER_BAR = 1e-6      # on the largest entry of E: the ceiling test_gpu_pose.py uses for P3P
# the scipy comparison: ten times the largest figure measured with this file (rotation 5.0e-6 degrees on the planar 300-match
# scene, translation direction 2.8e-5 degrees on the 40-match scene; BFGS with a numerical gradient stops that far from the minimum)
SCIPY_ROT_DEG = 5.0e-5
SCIPY_DIR_DEG = 2.8e-4


def _exact_rows(seed: int, n: int, planar: bool):
    """Noise-free normalised points of a planted pair -> (rows [n, 4], E planted, Frobenius norm 1)"""
    rng = np.random.default_rng(seed)
    R = PR.rodrigues(rng.uniform(-0.3, 0.3, 3))
    t = rng.uniform(-1.0, 1.0, 3)
    X = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.0, 12.0, n)], 1)
    if planar:
        X[:, 2] = 6.0 / (1.0 + 0.3 * X[:, 0] / 6.0 - 0.2 * X[:, 1] / 6.0)
    Y = X @ R.T + t
    E = (TR._skew(t) @ R).reshape(9)
    return np.concatenate([X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]], 1), E / np.linalg.norm(E)


def test_monomial_tables_are_what_the_kernel_holds():
    src = (ROOT / "pram_amd" / "csrc" / "twoview.hip").read_text()
    for name, tab in (("T11", TR.T11), ("T21", TR.T21)):
        body = re.search(name + r"\[\d+\]\[4\] = (\{.*?\}\});", src, re.S).group(1)
        assert [int(x) for x in re.findall(r"\d+", body)] == tab.reshape(-1).tolist()
    for name, val in (("BISECT", TR.BISECT), ("NEWTON", TR.NEWTON)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == val
    assert float(re.search(r"CHECK_TOL = ([0-9.e+-]+);", src).group(1)) == TR.CHECK_TOL
    assert float(re.search(r"RANK_EPS = ([0-9.e+-]+);", src).group(1)) == TR.RANK_EPS


def test_sampler_five_distinct_picks():
    for n in (5, 6, 17, 500):
        f = TR.sample_fives(3, 2, n, 2000)
        s = np.sort(f, 1)
        assert (s[:, 1:] != s[:, :-1]).all() and f.min() >= 0 and f.max() < n
        if n == 5:
            assert (s == np.arange(5)).all()
        if n >= 17:      # every index is drawn, and about equally often
            c = np.bincount(f.reshape(-1), minlength=n)
            assert c.min() > 0 and c.max() < 2.5 * c.mean()
    assert (TR.sample_fives(3, 2, 4, 10) == -1).all()
    assert not np.array_equal(TR.sample_fives(3, 2, 50, 10), TR.sample_fives(3, 3, 50, 10))


@pytest.mark.parametrize("planar", [False, True])
def test_solver_finds_the_planted_matrix(planar):
    """400 noise-free samples: the planted E, up to sign, is among the solutions within SOLVER_BAR; a sample is left out when the
    solver itself declares it degenerate (n_sol = 0: a pivot of the 5 x 9 system below RANK_EPS of the first, or a Sturm chain
    that is not finite), which may happen to 1 % at most.  Every solution satisfies the ten constraints and the five epipolar
    equations."""
    rows, Et = _exact_rows(11 + planar, 500, planar)
    E, ns, fives = TR.hypotheses(rows, 3, 0, 400)
    valid = np.arange(TR.MAX_SOL)[None] < ns[:, None]
    err = np.minimum(np.abs(E - Et).max(2), np.abs(E + Et).max(2))
    err = np.where(valid, err, np.inf).min(1)
    left = ns == 0
    print(f"planar = {planar}: median {np.median(err):.2e}, p99 {np.quantile(err[~left], 0.99):.2e}, worst {err[~left].max():.2e}, left out {left.sum()}")
    assert left.sum() <= 4 and err[~left].max() <= SOLVER_BAR
    assert (E[~valid] == 0.0).all() and np.allclose(np.sqrt((E[valid] ** 2).sum(1)), 1.0, atol=1e-14)
    assert TR.violation(E[valid]).max() <= TR.CHECK_TOL and np.median(TR.violation(E[valid])) < 1e-12
    s = rows[fives]      # [400, 5, 4]
    h0 = np.concatenate([s[:, :, 0:2], np.ones((400, 5, 1))], 2)
    h1 = np.concatenate([s[:, :, 2:4], np.ones((400, 5, 1))], 2)
    epi = np.einsum("tsa,tkab,tsb->tks", h1, E.reshape(400, TR.MAX_SOL, 3, 3), h0)
    print(f"   largest epipolar residual of a sample {np.abs(epi).max():.2e}")
    assert np.abs(epi).max() < 1e-9


def test_solver_refuses_degenerate_samples():
    rows, _ = _exact_rows(5, 20, False)
    dup = rows[[0, 0, 0, 0, 0, 1, 2, 3, 4, 5]].reshape(2, 5, 4)
    E, ns = TR.five_point(dup[:, :, 0:2], dup[:, :, 2:4])
    assert ns[0] == 0 and ns[1] >= 1 and not E[0].any()
    bad = rows.copy()
    bad[::2] = np.nan      # what pair_rows leaves for an index outside its frame
    E, ns, fives = TR.hypotheses(bad, 1, 0, 64)
    hit = (fives % 2 == 0).any(1)
    assert hit.any() and (~hit).any() and (ns[hit] == 0).all() and (ns[~hit] >= 1).all() and np.isfinite(E).all()
    E, ns, fives = TR.hypotheses(rows[:4], 1, 0, 8)
    assert (ns == 0).all() and (fives == -1).all()


@pytest.fixture(scope="module")
def runs():
    out = []
    for i, s in enumerate(TR.scenes()):
        rows, f0, f1 = TR.scene_rows(s)
        out.append((s, rows, f0, f1, TR.estimate_pair(rows, f0, f1, p=i)))
    return out


def test_restatement_keeps_the_planted_matches(runs):
    """Every scene has 40 matches at least: 95 % of the planted true matches are kept, the relative pose has det R = +1 and a unit
    translation, and the rule of the final support holds."""
    for s, rows, f0, f1, r in runs:
        true = ~s["outlier"]
        assert r["success"] and r["keep"][true].mean() >= 0.95, s["n"]
        assert r["num_inliers"] == r["keep"].sum() >= max(15, 0.1 * s["n"]) and r["num_inliers"] >= r["n0"] and r["num_front"] <= r["num_inliers"]
        assert abs(np.linalg.det(r["R"]) - 1.0) < 1e-12 and abs(np.linalg.norm(r["tvec"]) - 1.0) < 1e-12
        assert abs(np.linalg.norm(r["E"]) - 1.0) < 1e-12 and r["qvec"][0] >= 0.0
        assert r["num_front"] >= 0.7 * r["num_inliers"]      # the planted points are in front of both cameras


def test_margins(runs):
    """No Sampson residual within 1e-9 relative of the threshold, under the final model and under the best hypothesis: the device's
    masks and counts are then the restatement's exactly."""
    for s, rows, f0, f1, r in runs:
        for E in (r["E"], r["E_hyp"]):
            e = TR.sampson(E.reshape(1, 9), rows)[0]
            assert np.min(np.abs(e / r["thr2"] - 1.0)) > 1e-9, s["n"]


def test_decomposition_recovers_a_planted_pose():
    rng = np.random.default_rng(4)
    for _ in range(20):
        R, t = PR.rodrigues(rng.uniform(-1.0, 1.0, 3)), rng.standard_normal(3)
        t = t / np.linalg.norm(t)
        E = TR.essential_of(R, t) * rng.choice([-1.0, 1.0])
        cands = TR.decompose(E)
        assert all(abs(np.linalg.det(Rc) - 1.0) < 1e-12 for Rc, _ in cands)
        assert min(max(np.abs(Rc - R).max(), np.abs(tc - t).max()) for Rc, tc in cands) < 1e-12
        X = np.stack([rng.uniform(-2, 2, 30), rng.uniform(-2, 2, 30), rng.uniform(4, 9, 30)], 1)
        Y = X @ R.T + 0.5 * t
        rows = np.concatenate([X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]], 1)
        fronts = [int(TR.front_mask(Rc, tc, rows).sum()) for Rc, tc in cands]
        k = int(np.argmax(fronts))
        assert fronts[k] == 30 and np.abs(cands[k][0] - R).max() < 1e-12 and sorted(fronts)[-2] < 30


def test_lm_against_scipy(runs):
    """The restatement's two refinements against scipy's BFGS on the same Cauchy-Sampson cost, the same inlier set and the same
    start (the hypothesis): the angle between the two results."""
    worst = [0.0, 0.0]
    for s, rows, f0, f1, r in runs:
        scale = 0.5 * (1.0 / f0 + 1.0 / f1)
        m0 = TR.inlier_mask(r["E_hyp"], rows, r["thr2"])
        cands = TR.decompose(r["E_hyp"])
        R0, t0 = cands[int(np.argmax([int((TR.front_mask(R, t, rows) & m0).sum()) for R, t in cands]))]
        R1, t1 = TR.refine(rows, m0, *TR.refine(rows, m0, R0, t0, scale, 20), scale, 20)
        Rs, ts = TR.scipy_refine(rows, m0, R0, t0, scale)      # from the hypothesis, not from the restatement's result
        er = float(np.degrees(np.linalg.norm(R1 @ Rs.T - np.eye(3)) / np.sqrt(2.0)))      # small angles: the chord, not the arc cosine
        et = float(np.degrees(2.0 * np.arcsin(min(1.0, 0.5 * np.linalg.norm(t1 - ts)))))
        c0, c1 = TR.lm_pass(rows, m0, R0, t0, scale)[0], TR.lm_pass(rows, m0, R1, t1, scale)[0]
        print(f"n = {s['n']}, planar = {s['planar']}: cost {c0:.4f} -> {c1:.4f}; scipy's result is {er:.2e} deg away, its direction {et:.2e} deg; "
              f"error against the planted pose {TR.pose_errors(R1, t1, s)}, scipy's {TR.pose_errors(Rs, ts, s)}")
        assert c1 <= c0
        worst = [max(worst[0], er), max(worst[1], et)]
        assert er < SCIPY_ROT_DEG and et < SCIPY_DIR_DEG
        # accuracy against the planted pose: no worse than what scipy reaches on the same inlier set
        mine, theirs = TR.pose_errors(R1, t1, s), TR.pose_errors(Rs, ts, s)
        assert mine[0] <= theirs[0] + SCIPY_ROT_DEG and mine[1] <= theirs[1] + SCIPY_DIR_DEG
    print("worst", worst)


def test_restatement_failures():
    s = TR.scenes()[0]
    rows, f0, f1 = TR.scene_rows(s)
    for n in (0, 4):
        r = TR.estimate_pair(rows[:n], f0, f1)
        assert not r["success"] and r["keep"].shape == (n,) and not r["E"].any()
    r = TR.estimate_pair(rows[:5], f0, f1, trials=16)      # a model, and 5 inliers below min_num_inliers
    assert not r["success"] and r["best"] >= 0 and r["n0"] == 5
    assert TR.estimate_pair(rows[:5], f0, f1, trials=16, min_num_inliers=5, min_inlier_ratio=1.0)["success"]
    r = TR.estimate_pair(np.tile(rows[:1], (50, 1)), f0, f1, trials=16)
    assert not r["success"] and r["best"] == -1


def test_header_and_exports(hip_lib):
    from pram_amd import _lib, ops
    # exported == declared, by type, and PRAM_TWOVIEW_MAX_SOL == ops.TWOVIEW_MAX_SOL: tests/test_abi_contract_cpu.py
    assert sorted(ENTRIES) == sorted(n for n in _lib.exported_symbols() if n.startswith("pram_twoview_"))
    assert TR.MAX_SOL == ops.TWOVIEW_MAX_SOL
    assert ops.TWOVIEW_TRIAL_BYTES == 10 * 72 + 10 * 12 + 4      # 720 bytes of hypotheses per trial, then counts, sums and n_sol


def test_defaults_and_dispatch():
    from pram_amd._lib import PramHipError
    from pram_amd.localization import triangulation as TG
    from pram_amd.localization import twoview as TV
    assert TV.TWOVIEW_DEFAULTS == dict(max_error=4.0, trials=1024, seed=0, min_inlier_ratio=0.1, min_num_inliers=15, refine_iters=20,
                                       pair_chunk=256) == TR.DEFAULTS
    assert TG.DEFAULTS == dict(max_error=4.0, trials=128, seed=0, min_tri_angle=1.5, max_reproj_error=4.0)      # no key added
    with pytest.raises(TypeError, match="bogus"):
        TV.estimate_two_view({}, [], [], bogus=1)
    with pytest.raises(ValueError, match="trials"):
        TV.estimate_two_view({}, [], [], trials=0)
    s = TR.scenes()[0]
    with pytest.raises(PramHipError):
        TV.keypoint_table(s["frames"], s["cameras"], "cpu")
    with pytest.raises(ValueError, match="cameras"):
        TV.keypoint_table(s["frames"], s["cameras"][:1], "cuda")
    poses = (np.tile([1.0, 0, 0, 0], (2, 1)), np.zeros((2, 3)))
    args = (s["frames"], s["cameras"], poses, [(0, 1)], [s["matches"]], "cpu")
    with pytest.raises(PramHipError):      # both new names are accepted: the call gets as far as the device
        TG.triangulate_map(*args, estimate_two_view_geometries=True, twoview={"trials": 64})
    with pytest.raises(TypeError, match="bogus"):
        TG.triangulate_map(*args, estimate_two_view_geometries=True, twoview={"bogus": 1})
    with pytest.raises(TypeError, match="two_view"):
        TG.triangulate_map(*args, two_view=True)
    with pytest.raises(ValueError, match="twoview"):
        TG.triangulate_map(*args, twoview={"trials": 64})
    assert set(TG.TWOVIEW_MAP_DEFAULTS) == {"estimate_two_view_geometries", "twoview"}
