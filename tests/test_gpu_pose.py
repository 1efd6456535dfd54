"""The pose kernels (csrc/pose.hip) against the numpy restatement tests/pose_ref.py, stage by stage and end to end.
Measured deviations and the bars derived from them: profiles/pose_parity.md."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import helpers as H
from tests import pose_ref as PR

pytestmark = pytest.mark.gpu

# bars = ten times the largest deviation measured on an MI355X (profiles/pose_parity.md); P3P never above 1e-6 relative
P3P_BAR = 3e-15           # relative, per pose entry, scaled by 1 + |t|
E2E_Q_BAR = 1e-8          # qvec, absolute
E2E_T_BAR = 2e-8          # tvec, relative to 1 + |t|
PREPARE_BAR = 1e-15       # measured 0 (bit-equal): ten ulps of a value below 1
P3P_SEEDS = (1, 2, 3)     # tests/test_pose_cpu.py::test_p3p_near_degenerate_share checks these stay inside the 1 %
P3P_COND = 1e-6
SCIPY_ROT_DEG, SCIPY_CENTRE_M = 2.5e-3, 1.3e-4      # as in tests/test_pose_cpu.py


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _up(scenes, dev, t0=None):
    k, x, c = PR.pad_batch(scenes, t0)
    return torch.from_numpy(k).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)


def _cams(scenes, dev):
    from pram_amd.localization.pose import camera_table
    ids, params = camera_table([s["cam"] for s in scenes])
    return torch.from_numpy(ids).to(dev), torch.from_numpy(params).to(dev), [int(i) for i in ids]


def test_sampling_exact(dev):
    from pram_amd import ops
    counts = [3, 4, 5, 17, 500, 2048, 0, 2]
    P, t0 = len(counts), 2048
    pts = torch.zeros(P, t0, 2, dtype=torch.float64, device=dev)
    xyz = torch.zeros(P, t0, 3, dtype=torch.float64, device=dev)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    for seed in (0, 7, 2 ** 63 + 12345):
        _, n_sol, tri = ops.pose_hypotheses(pts, xyz, cnt, 777, seed, with_triples=True)
        tri = tri.cpu().numpy()
        assert not n_sol.any()      # all-zero rows: duplicates, no solution, no fault
        for p, n in enumerate(counts):
            if n < 3:
                assert (tri[p] == -1).all()
                continue
            ref = PR.sample_triples(seed, p, n, 777)
            assert np.array_equal(tri[p], ref), (seed, n)
            assert tri[p].max() < n and tri[p].min() >= 0
            assert (tri[p][:, 0] != tri[p][:, 1]).all() and (tri[p][:, 0] != tri[p][:, 2]).all() and (tri[p][:, 1] != tri[p][:, 2]).all()


def test_prepare_against_restatement(dev):
    from pram_amd import ops
    scenes = [PR.make_scene(40 + i, cam, n, 0.2) for i, (cam, n) in enumerate(zip(PR.SCENE_CAMERAS.values(), (300, 64, 1000, 17, 700)))]
    k, x, c = _up(scenes, dev)
    cm, cp, host = _cams(scenes, dev)
    pts = ops.pose_prepare(k, c, cm, cp, host, 1).cpu().numpy()
    worst = 0.0
    for i, s in enumerate(scenes):
        ref = PR.prepare(s["kpts"], *PR.camera_row(s["cam"]))
        worst = max(worst, float(np.abs(pts[i, :s["n"]] - ref).max()))
    print(f"prepare: largest deviation {worst:.3e}")
    assert worst <= PREPARE_BAR
    with pytest.raises(Exception, match="not supported"):
        ops.pose_prepare(k, c, cm, cp, [0, 1, 9, 3, 4], 1)


def _match_roots(dp, dn, rp, rn):
    """largest relative deviation between two root sets of one trial (roots matched by nearest t), inf if the counts differ"""
    if dn != rn:
        return math.inf
    worst = 0.0
    for k in range(rn):
        j = int(np.argmin(np.abs(dp[:dn, [3, 7, 11]] - rp[k, [3, 7, 11]]).sum(1)))
        worst = max(worst, float(np.abs(dp[j] - rp[k]).max() / (1.0 + np.abs(rp[k, [3, 7, 11]]).max())))
    return worst


def test_p3p_roots_against_restatement(dev):
    from pram_amd import ops
    s = PR.make_scene(11, PR.SCENE_CAMERAS["OPENCV"], 500, 0.3)
    k, x, c = _up([s], dev)
    cm, cp, host = _cams([s], dev)
    pts = ops.pose_prepare(k, c, cm, cp, host, 1)
    ref_pts = PR.prepare(s["kpts"], *PR.camera_row(s["cam"]))
    worst = 0.0
    for seed in P3P_SEEDS:
        poses, n_sol = ops.pose_hypotheses(pts, x, c, 1000, seed)
        poses, n_sol = poses.cpu().numpy()[0], n_sol.cpu().numpy()[0]
        rp, rn, cond = PR.hypotheses(ref_pts, s["xyz"], seed, 0, 1000, True)
        keep = cond >= P3P_COND
        assert (~keep).mean() < 0.01
        assert np.all(np.isfinite(poses))
        for h in np.nonzero(keep)[0]:
            d = _match_roots(poses[h], n_sol[h], rp[h], rn[h])
            assert d < 1e-6, (seed, h, d, n_sol[h], rn[h])
            worst = max(worst, d)
    print(f"p3p: largest relative deviation over {len(P3P_SEEDS)} x 1000 trials {worst:.3e}")
    assert worst <= P3P_BAR


def test_scoring_exact(dev):
    from pram_amd import ops
    scenes = [PR.make_scene(60 + i, cam, n, 0.5) for i, (cam, n) in enumerate(zip(PR.SCENE_CAMERAS.values(), (300, 2048, 1000, 40, 1700)))]
    k, x, c = _up(scenes, dev)
    cm, cp, host = _cams(scenes, dev)
    pts = ops.pose_prepare(k, c, cm, cp, host, 1)
    poses, n_sol = ops.pose_hypotheses(pts, x, c, 500, 3)
    h_inl, h_res, best = ops.pose_score(pts, x, c, poses, n_sol, cm, cp, 1, 4.0)
    pts, poses, n_sol, h_inl, h_res, best = (t.cpu().numpy() for t in (pts, poses, n_sol, h_inl, h_res, best))
    for i, s in enumerate(scenes):
        n = s["n"]
        th = 4.0 / PR.f_mean(*PR.camera_row(s["cam"]))
        thr2 = th * th
        flat = poses[i].reshape(-1, 12)
        valid = (np.arange(4)[None, :] < n_sol[i][:, None]).reshape(-1)
        # a condition on the input: no residual within 1e-9 relative of the threshold
        with np.errstate(all="ignore"):
            xc = np.einsum("mij,nj->mni", flat.reshape(-1, 3, 4)[:, :, :3], s["xyz"]) + flat.reshape(-1, 3, 4)[:, None, :, 3]
            e = (xc[..., 0] / xc[..., 2] - pts[i, None, :n, 0]) ** 2 + (xc[..., 1] / xc[..., 2] - pts[i, None, :n, 1]) ** 2
        assert not np.any(np.abs(e[valid] - thr2) <= 1e-9 * thr2)
        cnt, res = PR.score(pts[i, :n], s["xyz"], flat, thr2)
        assert np.array_equal(h_inl[i][valid], cnt[valid])
        assert (h_inl[i][~valid] == -1).all()
        assert np.allclose(h_res[i][valid], res[valid], rtol=1e-12, atol=0)
        assert best[i] == PR.rank(h_inl[i], h_res[i], valid)


@pytest.fixture(scope="module")
def e2e(dev):
    from pram_amd.localization.pose import estimate_poses
    scenes = PR.e2e_scenes()
    k, x, c = _up(scenes, dev)
    est = estimate_poses(k, x, c, [s["cam"] for s in scenes], seg_k=1, threshold=PR.E2E_THRESHOLD, trials=1000, refine_iters=20, seed=7)
    ref = [PR.estimate_pose(s["kpts"], s["xyz"], s["cam"], threshold=PR.E2E_THRESHOLD, trials=1000, refine_iters=20, seed=7, p=i)
           for i, s in enumerate(scenes)]
    return scenes, {kk: v.cpu().numpy() for kk, v in est.items()}, ref, (k, x, c)


def test_end_to_end_against_restatement_and_scipy(e2e):
    scenes, est, ref, _ = e2e
    wq = wt = 0.0
    for i, (s, r) in enumerate(zip(scenes, ref)):
        n = s["n"]
        assert bool(est["success"][i]) == r["success"] and r["success"]
        assert est["best"][i] == r["best"]
        assert np.array_equal(est["inliers"][i, :n].astype(bool), r["inliers"]) and not est["inliers"][i, n:].any()
        assert est["num_inliers"][i] == r["num_inliers"]
        dq = float(np.abs(est["qvec"][i] - r["qvec"]).max())
        dt = float(np.abs(est["tvec"][i] - r["tvec"]).max() / (1.0 + np.abs(r["tvec"]).max()))
        wq, wt = max(wq, dq), max(wt, dt)
        R = PR.qvec_to_rot(est["qvec"][i])
        er, ec = PR.pose_errors(R, est["tvec"][i], s["R"], s["t"])
        rr, rc = PR.pose_errors(r["R"], r["tvec"], s["R"], s["t"])
        # not worse than the restatement's own error by more than the device-restatement bar (as an angle / a length)
        assert er <= rr + math.degrees(4.0 * E2E_Q_BAR) + 1e-12 and ec <= rc + 4.0 * E2E_T_BAR * (1.0 + np.abs(r["tvec"]).max())
        Rs, ts = PR.scipy_refine(s, r["inliers"], s["R"], s["t"])
        sr, sc = PR.pose_errors(R, est["tvec"][i], Rs, ts)
        print(f"e2e {s['cam'][0]:15s} n {n:5d} inliers {r['num_inliers']:5d} dq {dq:.2e} dt {dt:.2e} | planted {er:.4f} deg {ec:.4f} m | scipy {sr:.2e} deg {sc:.2e} m")
        assert sr < SCIPY_ROT_DEG and sc < SCIPY_CENTRE_M
    print(f"e2e: largest qvec deviation {wq:.3e}, largest relative tvec deviation {wt:.3e}")
    assert wq <= E2E_Q_BAR and wt <= E2E_T_BAR


def test_determinism(e2e, dev):
    from pram_amd.localization.pose import estimate_poses
    scenes, est, _, (k, x, c) = e2e
    cams = [s["cam"] for s in scenes]
    again = estimate_poses(k, x, c, cams, seg_k=1, threshold=PR.E2E_THRESHOLD, trials=1000, refine_iters=20, seed=7)
    for kk in ("qvec", "tvec", "inliers", "num_inliers", "success", "best"):
        assert np.array_equal(again[kk].cpu().numpy(), est[kk]), kk
    # a pair inside a batch of 80 against the same pair alone: the sampler depends on the pair index, so the pair sits at
    # index 0 both times and 79 other pairs follow it
    big = [scenes[10]] + [scenes[(3 * j) % 15] for j in range(79)]
    kb, xb, cb = _up(big, dev)
    full = estimate_poses(kb, xb, cb, [s["cam"] for s in big], seg_k=1, threshold=PR.E2E_THRESHOLD, trials=1000, refine_iters=20, seed=9)
    alone = estimate_poses(kb[:1].contiguous(), xb[:1].contiguous(), cb[:1].contiguous(), [big[0]["cam"]], seg_k=1, threshold=PR.E2E_THRESHOLD,
                           trials=1000, refine_iters=20, seed=9)
    for kk in ("qvec", "tvec", "inliers", "num_inliers", "success", "best"):
        assert np.array_equal(full[kk][:1].cpu().numpy(), alone[kk].cpu().numpy()), kk


def test_failures_without_faults(dev):
    from pram_amd.localization.pose import estimate_poses
    cam = PR.SCENE_CAMERAS["RADIAL"]
    good = PR.make_scene(80, cam, 200, 0.3)
    rng = np.random.default_rng(5)

    def variant(n=200, **kw):
        s = dict(PR.make_scene(81, cam, max(n, 1), 0.0))
        s.update(n=n, kpts=s["kpts"][:n], xyz=s["xyz"][:n])
        s.update(kw)
        return s

    base = variant()
    cases = [variant(0), variant(1), variant(2),
             variant(kpts=np.stack([rng.uniform(0, 1024, 200), rng.uniform(0, 768, 200)], 1).astype(np.float32)),      # all rows outliers
             variant(xyz=base["xyz"] - 2.0 * (base["xyz"] + base["R"].T @ base["t"])),                                  # all behind the camera
             variant(xyz=np.outer(np.linspace(1.0, 9.0, 200), [0.3, -0.2, 1.0]) + [100.0, -300.0, 30.0]),               # collinear
             variant(xyz=np.repeat(base["xyz"][:1], 200, 0), kpts=np.repeat(base["kpts"][:1], 200, 0))]                 # duplicate rows
    scenes = [good] + cases + [good]
    k, x, c = _up(scenes, dev)
    # "no pose" for 200 arbitrary rows is a matter of min_inlier_ratio (any non-degenerate triple supports its own roots)
    est = estimate_poses(k, x, c, [cam] * len(scenes), seg_k=1, threshold=4.0, trials=300, min_inlier_ratio=0.3, seed=2)
    est = {kk: v.cpu().numpy() for kk, v in est.items()}
    for kk, v in est.items():
        assert np.all(np.isfinite(v.astype(np.float64))), kk
    for i in range(1, 8):
        assert est["success"][i] == 0 and est["num_inliers"][i] == 0 and not est["inliers"][i].any(), i
        assert not est["qvec"][i].any() and not est["tvec"][i].any()
    # the neighbours: bit-equal to the same pairs in a batch without the bad ones (pair index kept: 0)
    assert est["success"][0] == 1 and est["success"][8] == 1 and est["num_inliers"][0] >= 120
    # the same batch at the default ratio 0.01: a pair of arbitrary rows now "succeeds" on the 3 rows of some triple and goes through both
    # LM passes on a rank-deficient set; nothing but finiteness, consistency and untouched neighbours is promised
    dflt = {kk: v.cpu().numpy() for kk, v in estimate_poses(k, x, c, [cam] * len(scenes), seg_k=1, threshold=4.0, trials=300, seed=2).items()}
    for kk, v in dflt.items():
        assert np.all(np.isfinite(v.astype(np.float64))), kk
    assert np.array_equal(dflt["num_inliers"], dflt["inliers"].sum(1)) and not dflt["success"][1:4].any() and not dflt["success"][6:8].any()
    assert ((dflt["num_inliers"] >= 3) == (dflt["success"] == 1)).all()
    for kk in ("qvec", "tvec", "inliers", "num_inliers", "success"):
        assert np.array_equal(dflt[kk][0], est[kk][0]) and np.array_equal(dflt[kk][8], est[kk][8]), kk
    k1, x1, c1 = _up([good], dev, t0=k.shape[1])
    one = estimate_poses(k1, x1, c1, [cam], seg_k=1, threshold=4.0, trials=300, min_inlier_ratio=0.3, seed=2)
    for kk in ("qvec", "tvec", "inliers", "num_inliers", "success"):
        assert np.array_equal(one[kk].cpu().numpy()[0], est[kk][0]), kk


def test_selection(dev):
    from pram_amd import ops
    rng = np.random.default_rng(0)
    succ = np.concatenate([[[1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [0, 1, 1, 0, 1], [1, 0, 1, 1, 1]], rng.integers(0, 2, (59, 5))]).astype(np.int32)
    ninl = np.concatenate([[[10, 50, 70, 0, 0], [10, 30, 30, 5, 29], [0, 0, 0, 0, 0], [0, 50, 90, 0, 95], [20, 0, 45, 99, 1]], rng.integers(0, 80, (59, 5))]).astype(np.int32)
    ninl = ninl * succ
    out = ops.pose_select(torch.from_numpy(succ.reshape(-1)).to(dev), torch.from_numpy(ninl.reshape(-1)).to(dev), 5, 40).cpu().numpy()
    for b in range(succ.shape[0]):
        assert tuple(out[b]) == PR.select(succ[b], ninl[b], 40), b
    assert tuple(out[0]) == (1, 1, 1) and tuple(out[1]) == (1, 0, 1) and tuple(out[2]) == (-1, -1, -1)


def test_public_call(dev):
    """localize_candidates on the candidate tests' synthetic map, extended so that each reference frame's xyzs and the query
    keypoints are consistent with a planted camera per query (five different models over the six queries, seg_k = 5): every
    candidate's success, inlier mask, qvec and tvec, and the chosen candidate, equal the numpy restatement run on match_candidates'
    own trimmed output with the pair's index p = b * seg_k + w; the planted pose is recovered where the restatement recovers it;
    match_candidates before and after gives bit-equal results (it was only refactored)."""
    from pram_amd.localization import candidates as cd
    from pram_amd.localization.pose import localize_candidates
    from pram_amd.nets.gml import GML
    g = GML({})
    g.load_state_dict(H.gml_sd(), strict=True)
    g = g.to(dev).eval()
    m, qs = CR.plan_scene()
    planted = PR.plant_cameras(m, qs, seed=3)
    cams = [pl["cam"] for pl in planted]
    assert len({c[0] for c in cams}) == 5
    store = cd.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], m["start_sid"], device=dev)
    feats, seg = CR.batch_features(qs, dev)
    SEG_K, THR, MIN_INL, TRIALS, SEED = 5, 4.0, 30, 1000, 4
    kw = dict(seg_k=SEG_K, min_kpts=32)
    before = cd.match_candidates(feats, seg, store, g, **kw)
    res = localize_candidates(feats, seg, store, g, cams, threshold=THR, min_inliers=MIN_INL, trials=TRIALS, seed=SEED, **kw)
    after = cd.match_candidates(feats, seg, store, g, **kw)
    keys = [k for k in before[0][0] if k.startswith("matched_")] + ["n_matches", "matches0", "matching_scores0"]
    wq = wt = 0.0
    n_tracked = 0
    for b in range(len(qs)):
        succ, ninl = [], []
        for w in range(SEG_K):
            c0, c = cd.trim_candidate(before[b][w]), res[b]["candidates"][w]
            n = int(c0["n_matches"])      # the padded rows beyond n_matches are not written by anyone
            for k in keys:
                cut = (lambda t: t[:n]) if k.startswith("matched_") else (lambda t: t)
                assert torch.equal(cut(before[b][w][k]), cut(after[b][w][k])) and torch.equal(cut(before[b][w][k]), cut(c[k])), (b, w, k)
            r = PR.estimate_pose(c0["matched_keypoints"].cpu().numpy(), c0["matched_xyzs"].cpu().numpy(), cams[b], threshold=THR, trials=TRIALS,
                                 refine_iters=20, seed=SEED, p=b * SEG_K + w)
            succ.append(int(r["success"]))
            ninl.append(r["num_inliers"])
            assert c["success"] == r["success"], (b, w)
            assert c["num_inliers"] == r["num_inliers"], (b, w, c["num_inliers"], r["num_inliers"])
            assert np.array_equal(c["inliers"][:n].cpu().numpy().astype(bool), r["inliers"]) and not c["inliers"][n:].any(), (b, w)
            dq = float(np.abs(c["qvec"] - r["qvec"]).max())
            dt = float(np.abs(c["tvec"] - r["tvec"]).max() / (1.0 + np.abs(r["tvec"]).max()))
            print(f"public call: query {b} candidate {w} matches {n:4d} success {int(r['success'])} inliers {r['num_inliers']:4d} dq {dq:.2e} dt {dt:.2e}")
            assert dq <= E2E_Q_BAR and dt <= E2E_T_BAR, (b, w, dq, dt)
            wq, wt = max(wq, dq), max(wt, dt)
        kept, status, order = PR.select(succ, ninl, MIN_INL)
        r = res[b]
        assert r["success"] == (kept >= 0) and r["tracking_status"] == (None if status < 0 else bool(status)) and r["order"] == order
        if kept >= 0:
            c = r["candidates"][kept]
            assert r["reference_frame_id"] == c["reference_frame_id"] and r["sid"] == c["sid"] and r["num_inliers"] == ninl[kept]
            assert np.array_equal(r["qvec"], c["qvec"]) and np.array_equal(r["tvec"], c["tvec"])
            n = int(c["n_matches"])
            assert r["matched_keypoints"].shape[0] == n == r["inliers"].shape[0] and int(r["inliers"].sum()) == ninl[kept]
            assert torch.equal(r["matched_xyzs"], c["matched_xyzs"][:n])
        if status == 1:      # a tracked query stands at its planted camera (0.5 px noise, 30 inliers or more: as in test_pose_cpu.py)
            n_tracked += 1
            er, ec = PR.pose_errors(PR.qvec_to_rot(r["qvec"]), r["tvec"], planted[b]["R"], planted[b]["t"])
            print(f"public call: query {b} tracked by candidate {kept}: {er:.4f} deg, {ec:.4f} m from the planted camera")
            assert er < 1.0 and ec < 0.5
    print(f"public call: largest qvec deviation {wq:.3e}, largest relative tvec deviation {wt:.3e}, tracked queries {n_tracked}")
    assert n_tracked >= 3      # queries 0 .. 3 carry hundreds of twinned keypoints; 4 and 5 are background / empty


def test_ctypes_entries(hip_lib, dev):
    """The five entries through ctypes alone, with their error statuses."""
    L = hip_lib
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s = PR.make_scene(90, PR.SCENE_CAMERAS["PINHOLE"], 100, 0.2)
    k, x, c = _up([s, s], dev)
    cm, cp, _ = _cams([s], dev)
    P, t0, H_ = 2, 100, 64
    pts = torch.zeros(P, t0, 2, dtype=torch.float64, device=dev)
    poses = torch.zeros(P, H_, 4, 12, dtype=torch.float64, device=dev)
    n_sol, tri = torch.zeros(P, H_, dtype=torch.int32, device=dev), torch.zeros(P, H_, 3, dtype=torch.int32, device=dev)
    h_inl, h_res = torch.zeros(P, H_ * 4, dtype=torch.int32, device=dev), torch.zeros(P, H_ * 4, dtype=torch.float64, device=dev)
    best = torch.zeros(P, dtype=torch.int32, device=dev)
    qv, tv = torch.zeros(P, 4, dtype=torch.float64, device=dev), torch.zeros(P, 3, dtype=torch.float64, device=dev)
    inl = torch.zeros(P, t0, dtype=torch.uint8, device=dev)
    ninl, succ = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
    chosen = torch.zeros(1, 3, dtype=torch.int32, device=dev)
    host = (C.c_int * 1)(1)
    bad = (C.c_int * 1)(7)
    d, nul = C.c_double, C.c_void_p(None)
    assert L.pram_pose_prepare(p(k), p(c), p(cm), p(cp), host, 1, 2, t0, p(pts), st) == 0
    assert L.pram_pose_prepare(p(k), p(c), p(cm), p(cp), bad, 1, 2, t0, p(pts), st) == -3      # PRAM_E_UNSUPPORTED
    assert L.pram_pose_prepare(nul, p(c), p(cm), p(cp), host, 1, 2, t0, p(pts), st) == -1
    assert L.pram_pose_prepare(p(k), p(c), p(cm), p(cp), host, 1, 0, t0, p(pts), st) == -1      # seg_k < 1
    assert L.pram_pose_prepare(p(k), p(c), p(cm), p(cp), host, -1, 2, t0, p(pts), st) == -1
    assert L.pram_pose_hypotheses(p(pts), p(x), p(c), P, t0, H_, C.c_ulonglong(5), p(poses), p(n_sol), p(tri), st) == 0
    assert L.pram_pose_hypotheses(p(pts), p(x), p(c), P, t0, 0, C.c_ulonglong(5), p(poses), p(n_sol), nul, st) == -1      # trials < 1
    assert L.pram_pose_hypotheses(p(pts), nul, p(c), P, t0, H_, C.c_ulonglong(5), p(poses), p(n_sol), nul, st) == -1
    assert L.pram_pose_score(p(pts), p(x), p(c), p(poses), p(n_sol), p(cm), p(cp), P, 2, t0, H_, d(4.0), p(h_inl), p(h_res), p(best), st) == 0
    assert L.pram_pose_score(p(pts), p(x), p(c), p(poses), p(n_sol), p(cm), p(cp), P, 0, t0, H_, d(4.0), p(h_inl), p(h_res), p(best), st) == -1
    assert L.pram_pose_score(p(pts), p(x), p(c), p(poses), p(n_sol), p(cm), p(cp), P, 2, t0, 0, d(4.0), p(h_inl), p(h_res), p(best), st) == -1
    assert L.pram_pose_refine(p(k), p(pts), p(x), p(c), p(poses), p(h_inl), p(best), p(cm), p(cp), P, 2, t0, H_, d(4.0), d(0.01), 10, p(qv), p(tv),
                              p(inl), p(ninl), p(succ), st) == 0
    assert L.pram_pose_refine(p(k), p(pts), p(x), p(c), p(poses), p(h_inl), p(best), p(cm), p(cp), P, 2, t0, H_, d(4.0), d(0.01), 10, nul, p(tv),
                              p(inl), p(ninl), p(succ), st) == -1
    assert L.pram_pose_refine(p(k), p(pts), p(x), p(c), p(poses), p(h_inl), p(best), p(cm), p(cp), P, 2, t0, H_, d(4.0), d(0.01), -1, p(qv), p(tv),
                              p(inl), p(ninl), p(succ), st) == -1
    assert L.pram_pose_select(p(succ), p(ninl), 1, 2, 12, p(chosen), st) == 0
    assert L.pram_pose_select(p(succ), p(ninl), 1, 0, 12, p(chosen), st) == -1
    assert L.pram_pose_select(nul, p(ninl), 1, 2, 12, p(chosen), st) == -1
    torch.cuda.synchronize()
    assert b"pram_pose_select" in L.pram_last_error()
    # the two pairs hold the same rows but are sampled differently: both find the planted pose
    r0 = PR.estimate_pose(s["kpts"], s["xyz"], s["cam"], threshold=4.0, trials=H_, refine_iters=10, seed=5, p=0)
    assert succ.tolist() == [1, 1] and ninl[0].item() == r0["num_inliers"]
    assert np.abs(qv[0].cpu().numpy() - r0["qvec"]).max() <= E2E_Q_BAR
    assert tuple(chosen[0].tolist()) == PR.select([1, 1], ninl.tolist(), 12)
    assert np.array_equal(tri[0].cpu().numpy(), PR.sample_triples(5, 0, 100, H_))
