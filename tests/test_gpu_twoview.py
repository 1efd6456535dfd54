"""GPU: two-view geometry without poses (pram_amd.localization.twoview, csrc/twoview.hip) against the numpy restatement
tests/twoview_ref.py, stage by stage and end to end, on the planted scenes (tests/test_twoview_cpu.py asserts the margins that make
the discrete results here exact), the failure cases, the output layout, the run through triangulate_map and the C entries.
profiles/twoview_parity.md has the measured deviations behind the bars."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pose_ref as PR
from tests import triangulation_ref as TRI
from tests import twoview_ref as TR

pytestmark = pytest.mark.gpu

# Largest entry of E, up to sign, between a device solution and the nearest solution of the restatement.  Measured on the MI355X
# over 3 seeds x 1000 trials: median 2.6e-14, p99 1.0e-9, worst 1.21e-7 with no trial left out; ten times that is above the
# ceiling of 1e-6, so the ceiling is the bar.
SOLVER_BAR = 1e-6
# End to end, device against restatement (measured worst over the eight scenes: E 3.25e-10, qvec 2.23e-10, tvec 5.59e-10; the
# Levenberg-Marquardt iterations amplify the last-bit differences of the reductions), times ten.
E_BAR, Q_BAR, T_BAR = 3.3e-9, 2.3e-9, 5.6e-9
POSE_BAR_DEG = 1e-6      # on the error against the planted pose, in degrees: T_BAR in radians is 3.2e-7 degrees, rounded up
MAP_MIN_INLIERS = 10     # the scene's pairs hold 66 to 93 matches of which about 90 % are true: every pair qualifies with room
MAP_TRIALS = 128


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def TV():
    from pram_amd.localization import twoview
    return twoview


@pytest.fixture(scope="module")
def TG():
    from pram_amd.localization import triangulation
    return triangulation


def _csr(TG, table, pairs, matches, dev):
    """-> the five device tensors every entry reads, and (Pn, M)"""
    use, pr, off, flat = TG._match_csr(table, pairs, matches)
    return (table["norm05"], table["frame_off"], TG._up(pr, dev), TG._up(off, dev), TG._up(flat, dev)), len(use), flat.shape[0]


@pytest.fixture(scope="module")
def planted(TV, dev):
    """The planted scenes as one batch, their restatement (computed once) and the device's result."""
    sc = TR.scenes()
    frames, cameras, pairs, matches = TR.batch(sc)
    table = TV.keypoint_table(frames, cameras, dev)
    ref = []
    for i, s in enumerate(sc):
        rows, f0, f1 = TR.scene_rows(s)
        ref.append(TR.estimate_pair(rows, f0, f1, p=i))
    return sc, table, pairs, matches, ref, TV.estimate_two_view(table, pairs, matches)


def test_sampler_equals_the_restatement(TV, TG, dev):
    from pram_amd import ops
    counts = [0, 4, 5, 6, 17, 64, 65, 500, 2048]
    rng = np.random.RandomState(0)
    frames = [{"keypoints": rng.uniform(0, 600, (2048, 2)).astype(np.float32)} for _ in range(2)]
    table = TV.keypoint_table(frames, [PR.SCENE_CAMERAS["PINHOLE"]] * 2, dev)
    off = np.zeros(len(counts) + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    m = np.concatenate([np.stack([np.arange(c), np.arange(c)], 1) for c in counts]).astype(np.int32)
    pr = np.tile(np.array([[0, 1]], dtype=np.int32), (len(counts), 1))
    for seed in (0, 12345, 2 ** 63 + 5):
        h = ops.twoview_hypotheses(table["norm05"], table["frame_off"], TG._up(pr, dev), TG._up(off, dev), TG._up(m, dev), 2, len(counts),
                                   m.shape[0], first_pair=3, trials=777, seed=seed, return_fives=True)
        fives, n_sol = h["fives"].cpu().numpy(), h["n_sol"].cpu().numpy()
        for k, n in enumerate(counts):
            assert np.array_equal(fives[k], TR.sample_fives(seed, 3 + k, n, 777)), (seed, n)
            if n < 5:
                assert (fives[k] == -1).all() and (n_sol[k] == 0).all()
            else:
                srt = np.sort(fives[k], 1)
                assert (srt[:, 1:] != srt[:, :-1]).all() and srt.min() >= 0 and srt.max() < n


def test_solver_against_the_restatement(TV, TG, dev):
    """One 500-match scene, 3 seeds x 1000 trials: the same number of solutions per trial, every solution within SOLVER_BAR of its
    nearest, up to sign; a trial whose counts differ is what is left out as ill-conditioned (a root whose constraint check sits at
    CHECK_TOL), and that share stays below 1 %."""
    from pram_amd import ops
    s = TR.make_scene(900, PR.SCENE_CAMERAS["PINHOLE"], PR.SCENE_CAMERAS["OPENCV"], 500, 0.0, False, noise_px=0.5)
    frames, cameras, pairs, matches = TR.batch([s])
    table = TV.keypoint_table(frames, cameras, dev)
    views, Pn, M = _csr(TG, table, pairs, matches, dev)
    rows, _, _ = TR.scene_rows(s)
    worst, left, total = 0.0, 0, 0
    for seed in (1, 2, 2 ** 63 + 5):
        h = ops.twoview_hypotheses(*views, 2, Pn, M, trials=1000, seed=seed)
        Ed, nd = h["E"].cpu().numpy()[0], h["n_sol"].cpu().numpy()[0]
        E, ns, _ = TR.hypotheses(rows, seed, 0, 1000)
        assert np.isfinite(Ed).all() and nd.min() >= 0 and nd.max() <= TR.MAX_SOL
        assert all((Ed[t, nd[t]:] == 0.0).all() for t in range(1000))
        nrm = np.sqrt((Ed ** 2).sum(2))
        assert np.all(np.abs(nrm[np.arange(TR.MAX_SOL)[None] < nd[:, None]] - 1.0) < 1e-14)
        same = ns == nd
        left, total = left + int((~same).sum()), total + 1000
        for t in np.nonzero(same & (ns > 0))[0]:
            a, b = E[t, :ns[t]], Ed[t, :ns[t]]
            d = np.minimum(np.abs(a[:, None] - b[None]).max(2), np.abs(a[:, None] + b[None]).max(2))
            worst = max(worst, float(d.min(1).max()))
    print(f"solver: worst deviation {worst:.3e}, trials left out {left} of {total}")
    assert left <= 0.01 * total and worst <= SOLVER_BAR


@pytest.mark.parametrize("n", [40, 300, 768, 769, 1700, 2048])      # 768 / 769: the last row of an LDS chunk and one past it
def test_scoring_equals_the_restatement(TV, TG, dev, n):
    """The device's own hypotheses scored by both: counts and best slot equal (no residual within 1e-9 relative of the threshold,
    asserted), residual sums to rtol 1e-12."""
    from pram_amd import ops
    s = TR.make_scene(1000 + n, PR.SCENE_CAMERAS["RADIAL"], PR.SCENE_CAMERAS["SIMPLE_RADIAL"], n, 0.3)
    frames, cameras, pairs, matches = TR.batch([s])
    table = TV.keypoint_table(frames, cameras, dev)
    views, Pn, M = _csr(TG, table, pairs, matches, dev)
    h = ops.twoview_hypotheses(*views, 2, Pn, M, trials=256, seed=7)
    sc = ops.twoview_score(*views, table["cam_model"], table["cam_params"], 2, Pn, M, h["E"], h["n_sol"], 4.0)
    rows, f0, f1 = TR.scene_rows(s)
    thr2 = TR.threshold2(4.0, f0, f1)
    E, ns = h["E"].cpu().numpy()[0], h["n_sol"].cpu().numpy()[0]
    cnt, res = TR.score(E, ns, rows, thr2)
    e = TR.sampson(E.reshape(-1, 9)[cnt >= 0], rows)
    assert np.nanmin(np.abs(e / thr2 - 1.0)) > 1e-9
    got_c, got_r = sc["h_inliers"].cpu().numpy().reshape(-1), sc["h_resid"].cpu().numpy().reshape(-1)
    assert np.array_equal(got_c, cnt) and (cnt == -1).sum() == (TR.MAX_SOL * 256 - ns.sum())
    assert np.allclose(got_r, res, rtol=1e-12, atol=0.0)
    assert int(sc["best"].cpu()[0]) == PR.rank(cnt, res, cnt >= 0) >= 0


def test_end_to_end_equals_the_restatement(planted):
    sc, _, _, _, ref, got = planted
    assert got["pair_index"].tolist() == list(range(len(sc))) and got["success"].all()
    for i, (s, r) in enumerate(zip(sc, ref)):
        assert r["success"] and np.array_equal(got["keep"][i], r["keep"]), s["n"]
        assert got["num_inliers"][i] == r["num_inliers"] and got["num_front"][i] == r["num_front"]
        assert np.array_equal(got["kept"][i], s["matches"][r["keep"]])
        assert got["inlier_ratio"][i] == r["num_inliers"] / s["n"]
        dE = min(np.abs(got["E"][i] - r["E"]).max(), np.abs(got["E"][i] + r["E"]).max())
        dq, dt = np.abs(got["qvec"][i] - r["qvec"]).max(), np.abs(got["tvec"][i] - r["tvec"]).max()
        print(f"n = {s['n']}: E {dE:.2e}, qvec {dq:.2e}, tvec {dt:.2e}")
        assert dE <= E_BAR and dq <= Q_BAR and dt <= T_BAR
        err_d, err_r = TR.pose_errors(PR.qvec_to_rot(got["qvec"][i]), got["tvec"][i], s), TR.pose_errors(r["R"], r["tvec"], s)
        assert err_d[0] <= err_r[0] + POSE_BAR_DEG and err_d[1] <= err_r[1] + POSE_BAR_DEG
        assert abs(np.linalg.norm(got["tvec"][i]) - 1.0) < 1e-12 and abs(np.linalg.norm(got["E"][i]) - 1.0) < 1e-12


def test_determinism_batch_position_and_chunks(TV, dev, planted):
    sc, table, pairs, matches, _, got = planted
    keys = ("E", "qvec", "tvec", "num_inliers", "num_front", "success", "inlier_ratio")
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in keys) and all(np.array_equal(x, y) for x, y in zip(a["keep"], b["keep"]))
    assert same(got, TV.estimate_two_view(table, pairs, matches))
    for chunk in (1, 7):      # 256 is the default: ``got``
        assert same(got, TV.estimate_two_view(table, pairs, matches, pair_chunk=chunk)), chunk
    # the pair at position 0 of an 80-pair batch equals the same pair alone
    s = sc[0]
    frames, cameras = s["frames"] * 80, s["cameras"] * 80
    t80 = TV.keypoint_table(frames, cameras, dev)
    many = TV.estimate_two_view(t80, [(2 * i, 2 * i + 1) for i in range(80)], [s["matches"]] * 80, trials=128)
    one = TV.estimate_two_view(t80, [(0, 1)], [s["matches"]], trials=128)
    assert all(np.array_equal(many[k][0], one[k][0]) for k in keys) and np.array_equal(many["keep"][0], one["keep"][0])


def test_failures_without_faults(TV, dev, planted):
    sc = planted[0]
    s0 = sc[3]
    n0 = s0["n"]
    rot = TR.make_scene(77, PR.SCENE_CAMERAS["PINHOLE"], PR.SCENE_CAMERAS["PINHOLE"], 200, 0.2, rotation_only=True)
    out = TR.make_scene(78, PR.SCENE_CAMERAS["PINHOLE"], PR.SCENE_CAMERAS["PINHOLE"], 200, 1.0)
    assert TV.estimate_two_view(TV.keypoint_table(s0["frames"], s0["cameras"], dev), np.zeros((0, 2), int), [])["success"].shape == (0,)
    bad = s0["matches"].copy()
    bad[::7, 0], bad[3::11, 1] = -1, n0
    good = s0["matches"]
    # every case between two copies of the good pair, each on frames of its own (a repeated pair of frames would be skipped)
    cases = [("good", s0, good), ("no matches", s0, np.zeros((0, 2), int)), ("four", s0, good[:4]), ("five", s0, good[:5]),
             ("identical", s0, np.tile(good[:1], (50, 1))), ("bad indices", s0, bad), ("rotation", rot, rot["matches"]),
             ("outliers", out, out["matches"]), ("outliers", TR.make_scene(79, *out["cameras"], 300, 1.0), None), ("good", s0, good)]
    frames, cameras, pairs, matches = [], [], [], []
    for name, s, m in cases:
        pairs.append((len(frames), len(frames) + 1))
        frames, cameras = frames + s["frames"], cameras + s["cameras"]
        matches.append(s["matches"] if m is None else m)
    k = len(frames)      # a pair naming the same frame twice
    pairs.append((0, 0)); matches.append(good)
    table = TV.keypoint_table(frames, cameras, dev)
    r = TV.estimate_two_view(table, pairs, matches)
    alone = TV.estimate_two_view(table, pairs[:1], matches[:1])
    assert all(np.isfinite(r[key]).all() for key in ("E", "qvec", "tvec")) and k == 20
    # the good pair is untouched by its neighbours; at position 9 it draws other samples and still finds the planted matches
    assert all(np.array_equal(r[key][0], alone[key][0]) for key in ("E", "qvec", "tvec", "num_inliers", "num_front", "success"))
    assert r["success"][0] and np.array_equal(r["keep"][0], alone["keep"][0])
    assert r["success"][9] and r["keep"][9][~s0["outlier"]].mean() >= 0.95
    for i in (1, 2, 3, 4, 7, 8):      # no matches, four, five (below min_num_inliers), identical (rank-deficient), all outliers
        assert not r["success"][i] and r["num_inliers"][i] == 0 and r["num_front"][i] == 0, cases[i][0]
        assert not r["E"][i].any() and not r["qvec"][i].any() and not r["tvec"][i].any() and not r["keep"][i].any() and len(r["kept"][i]) == 0
    assert np.isnan(r["inlier_ratio"][1]) and (r["inlier_ratio"][[2, 3, 4, 7, 8]] == 0).all()
    # indices of -1 and n: never inliers, the rest of the pair is found
    in_range = (bad[:, 0] >= 0) & (bad[:, 1] < n0)
    assert r["success"][5] and not r["keep"][5][~in_range].any() and r["keep"][5].sum() >= 0.9 * (alone["keep"][0] & in_range).sum()
    # a pure rotation: the rotation and the mask are meaningful, the translation is not
    assert r["success"][6] and r["keep"][6][~rot["outlier"]].mean() >= 0.95
    c = np.clip((np.trace(PR.qvec_to_rot(r["qvec"][6]) @ rot["R"].T) - 1.0) / 2.0, -1.0, 1.0)
    assert np.degrees(np.arccos(c)) < 0.5
    # the same frame twice: finite, and whatever it decides it keeps the layout
    assert len(r["keep"][10]) == n0 and r["keep"][10].sum() == len(r["kept"][10])


def test_output_layout(TV, TG, dev, planted):
    """What the triangulation tests assert of pram_tri_verify: kept holds the kept matches in original order from match_off[p] on,
    edges is -1 where dropped and names the rows elsewhere, count is right."""
    sc, table, pairs, matches, ref, _ = planted
    v = TV._estimate(table, pairs, matches, TV._twoview_params("test", {}))
    off, fo = v["match_off"], table["frame_off_host"]
    keep, kept, edges, count = (v[k].cpu().numpy() for k in ("keep", "kept", "edges", "count"))
    for p, (s, r) in enumerate(zip(sc, ref)):
        a, b = off[p], off[p + 1]
        m = s["matches"]
        assert count[p] == r["num_inliers"] and np.array_equal(keep[a:b].astype(bool), r["keep"])
        assert np.array_equal(kept[a:a + count[p]], m[r["keep"]])
        want = np.where(r["keep"][:, None], m + np.array([fo[2 * p], fo[2 * p + 1]]), -1)
        assert np.array_equal(edges[a:b], want)
    # the slot the finish read: the restatement's best, pair by pair
    from pram_amd import ops
    views, Pn, M = _csr(TG, table, pairs, matches, dev)
    h = ops.twoview_hypotheses(*views, table["n_frames"], Pn, M)
    best = ops.twoview_score(*views, table["cam_model"], table["cam_params"], table["n_frames"], Pn, M, h["E"], h["n_sol"])["best"]
    assert best[:Pn].cpu().tolist() == [r["best"] for r in ref]


def test_through_the_map(TG, dev):
    """triangulate_map with the estimator in the place of stage 2 (min_num_inliers = MAP_MIN_INLIERS): every pair's mask equals the
    restatement's, the points go through mapbuild.track_tables, and the masks do not move when the poses do, where the known-pose
    verification loses more than half of the true matches.  The default call is what its stages give one by one."""
    from pram_amd.localization import mapbuild
    s = TRI.tri_scene()
    args = (s["frames"], s["cameras"])
    tv = {"min_num_inliers": MAP_MIN_INLIERS, "trials": MAP_TRIALS}
    res = TG.triangulate_map(*args, (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev, estimate_two_view_geometries=True, twoview=tv)
    use = TRI.unique_pairs(s["pairs"])
    assert res["pair_index"].tolist() == list(use)
    fm = [PR.f_mean(int(m), p) for m, p in zip(s["cam_model"], s["cam_params"])]
    two = res["two_view"]
    for p, k in enumerate(use):
        a, b = s["pairs"][k]
        r = TR.estimate_pair(TR.pair_rows(s["norm05"], s["frame_off"], a, b, s["matches"][k]), fm[a], fm[b], p=p, **tv)
        assert np.array_equal(two["keep"][p], r["keep"]) and bool(two["success"][p]) == r["success"] and two["num_inliers"][p] == r["num_inliers"], p
    assert two["success"][:-1].all() and not two["success"][-1] and two["E"].shape == (len(use), 9)
    assert len(res["point_ids"]) >= 250 and np.isfinite(res["point3D_xyzs"]).all()
    tab = mapbuild.track_tables(SimpleNamespace(frame_ids=np.arange(len(s["frames"]))), res["tracks"])
    assert np.array_equal(tab["point_ids"], res["point_ids"]) and tab["trk_frame"].min() >= 0
    # every pose rotated by 10 degrees about an axis of its own: the poses no longer explain the matches
    rng = np.random.RandomState(3)
    q2 = []
    for q in s["qvec"]:
        ax = rng.normal(size=3)
        q2.append(PR.rot_to_qvec(PR.rodrigues(np.radians(10.0) * ax / np.linalg.norm(ax)) @ PR.qvec_to_rot(q / np.linalg.norm(q))))
    q2 = np.array(q2)
    moved = TG.triangulate_map(*args, (q2, s["tvec"]), s["pairs"], s["matches"], dev, estimate_two_view_geometries=True, twoview=tv)
    assert all(np.array_equal(x, y) for x, y in zip(moved["two_view"]["keep"], two["keep"]))
    assert all(np.array_equal(moved["two_view"][k], two[k]) for k in ("E", "qvec", "tvec", "num_inliers", "num_front", "success"))
    t_good, t_moved = TG.frame_table(*args, (s["qvec"], s["tvec"]), dev), TG.frame_table(*args, (q2, s["tvec"]), dev)
    v_good, v_moved = TG.verify_matches(t_good, s["pairs"], s["matches"]), TG.verify_matches(t_moved, s["pairs"], s["matches"])
    n_good, n_moved = sum(int(k.sum()) for k in v_good["keep"]), sum(int((k & g).sum()) for k, g in zip(v_moved["keep"], v_good["keep"]))
    print(f"known-pose verification keeps {n_good} matches at the true poses, {n_moved} of them at the rotated ones; the estimator keeps "
          f"{sum(int(k.sum()) for k in two['keep'])} at both")
    assert n_moved < 0.5 * n_good
    # the default call: no estimator, and the stages' own results
    base = TG.triangulate_map(*args, (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev)
    assert "two_view" not in base and np.array_equal(base["inlier_ratio"], v_good["inlier_ratio"], equal_nan=True)
    edges = np.concatenate([np.stack([t_good["frame_off_host"][a] + k[:, 0], t_good["frame_off_host"][b] + k[:, 1]], 1)
                            for (a, b), k in zip(s["pairs"][v_good["pair_index"]], v_good["kept"])])
    trk = TG.build_tracks(t_good, edges)
    want = TG.map_tables(np.arange(len(s["frames"])), t_good["frame_off_host"], trk, TG.triangulate_tracks(t_good, trk))
    assert np.array_equal(base["point_ids"], want["point_ids"]) and np.array_equal(base["point3D_xyzs"], want["point3D_xyzs"])
    assert all(np.array_equal(base["tracks"][i][1], want["tracks"][i][1]) for i in want["tracks"])


def test_ctypes_entries(TV, TG, dev, hip_lib):
    """One small call per entry through the C ABI, and what each refuses."""
    L = hip_lib
    s = TR.scenes()[0]
    frames, cameras, pairs, matches = TR.batch([s])
    table = TV.keypoint_table(frames, cameras, dev)
    (norm, fo, pr, off, flat), Pn, M = _csr(TG, table, pairs, matches, dev)
    T_ = 64
    p = lambda t: C.c_void_p(t.data_ptr())
    st, nul, d = C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(None), C.c_double
    z = lambda *sh, dt=torch.float64: torch.zeros(*sh, dtype=dt, device=dev)
    i32 = torch.int32
    E, n_sol, fives = z(1, T_, 10, 9), z(1, T_, dt=i32), z(1, T_, 5, dt=i32)
    h_inl, h_res, best = z(1, T_, 10, dt=i32), z(1, T_, 10), z(1, dt=i32)
    Eo, qv, tv, ninl, nfr, succ, cnt = z(1, 9), z(1, 4), z(1, 3), z(1, dt=i32), z(1, dt=i32), z(1, dt=i32), z(1, dt=i32)
    keep, kept, edges = z(M, dt=torch.uint8), z(M, 2, dt=i32), z(M, 2, dt=i32)
    cm, cp = table["cam_model"], table["cam_params"]
    a = (p(norm), p(fo), p(pr), p(off), p(flat))
    assert L.pram_twoview_hypotheses(*a, 2, 1, M, 0, T_, C.c_ulonglong(5), p(E), p(n_sol), p(fives), st) == 0
    assert L.pram_twoview_hypotheses(*a, 2, 1, M, 0, 0, C.c_ulonglong(5), p(E), p(n_sol), nul, st) == -1      # trials < 1
    assert L.pram_twoview_hypotheses(*a, 2, 1, M, -1, T_, C.c_ulonglong(5), p(E), p(n_sol), nul, st) == -1      # first_pair < 0
    assert L.pram_twoview_hypotheses(*a, 2, 1, M, 0, T_, C.c_ulonglong(5), nul, p(n_sol), nul, st) == -1
    assert L.pram_twoview_score(*a, p(cm), p(cp), 2, 1, M, p(E), p(n_sol), T_, d(4.0), p(h_inl), p(h_res), p(best), st) == 0
    assert L.pram_twoview_score(*a, p(cm), p(cp), 2, 1, M, p(E), p(n_sol), T_, d(0.0), p(h_inl), p(h_res), p(best), st) == -1      # max_error
    assert L.pram_twoview_score(*a, p(cm), nul, 2, 1, M, p(E), p(n_sol), T_, d(4.0), p(h_inl), p(h_res), p(best), st) == -1
    fin = lambda iters, q: L.pram_twoview_finish(*a, p(cm), p(cp), 2, 1, M, p(E), p(h_inl), p(best), T_, d(4.0), d(0.1), 15, iters, p(Eo), q, p(tv),
                                                 p(ninl), p(nfr), p(succ), p(keep), p(kept), p(edges), p(cnt), st)
    assert fin(10, p(qv)) == 0
    assert fin(-1, p(qv)) == -1 and fin(10, nul) == -1
    torch.cuda.synchronize()
    assert b"pram_twoview_finish" in L.pram_last_error()
    rows, f0, f1 = TR.scene_rows(s)
    r = TR.estimate_pair(rows, f0, f1, p=0, trials=T_, seed=5, refine_iters=10)
    assert np.array_equal(fives.cpu().numpy()[0], TR.sample_fives(5, 0, s["n"], T_))
    assert succ.item() == 1 and ninl.item() == r["num_inliers"] == cnt.item() and int(best.item()) == r["best"]
    assert np.array_equal(keep.cpu().numpy().astype(bool), r["keep"]) and np.abs(qv.cpu().numpy()[0] - r["qvec"]).max() <= Q_BAR
