"""CPU: the numpy restatement of the mapper's glue (tests/mapper_ref.py) on its own, the two host utilities, the header and the
exports, the host logic of pram_amd.localization.mapper on a stub, and the margins that make the discrete comparisons of
tests/test_gpu_mapper.py exact."""
from pathlib import Path

import numpy as np
import pytest

from tests import mapper_ref as MR
from tests import pose_ref as PR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_map_pair_angles_workspace_bytes", "pram_map_pair_angles", "pram_map_seed", "pram_map_correspond", "pram_map_choose",
           "pram_map_pack", "pram_map_live_edges")


# ---------------------------------------------------------------- the restatement on its own
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 1000, 1001])
def test_lower_median_is_the_sorted_element(n):
    rng = np.random.RandomState(n)
    for case in range(4):
        a = rng.uniform(0.0, np.pi, size=n)
        if case == 1:
            a = np.round(a, 1)                    # ties
        if case == 2:
            a[:] = a[0]                           # all equal
        if case == 3:
            a[rng.uniform(size=n) < 0.3] = np.nan      # matches that do not count
            a[rng.randint(n)] = 0.0                    # an angle of exactly 0 counts
        live = np.sort(a[~np.isnan(a)])
        cnt, med = MR.lower_median(a)
        assert cnt == len(live) and med == live[(len(live) - 1) // 2]
        assert MR.bisect_median(a) == med
    assert MR.lower_median(np.full(3, np.nan)) == (0, 0.0) and MR.bisect_median(np.full(3, np.nan)) == 0.0
    assert MR.lower_median(np.zeros(0)) == (0, 0.0)


def test_match_angles_against_planted_geometry():
    """The angle is the angle between the two planted rays, the midpoint's depths are the planted depths."""
    s = MR.planted_scene()
    i = s["pairs"].tolist().index([2, 5])
    q, t = MR.true_relative(s, 2, 5)
    m = s["matches"][i]
    ang = MR.match_angles(s["norm05"], s["frame_off"], 2, 5, m, q, t)
    C = s["table"][:, 12:15]
    right = {(s["where"][(2, pt)], s["where"][(5, pt)]): pt for pt in range(MR.N_POINTS) if (2, pt) in s["where"] and (5, pt) in s["where"]}
    errs = []
    for e, (a, b) in enumerate(m.tolist()):
        if (a, b) in right:
            X = s["xyz"][right[(a, b)]]
            r0, r1 = X - C[2], X - C[5]
            true = np.arccos(r0 @ r1 / np.linalg.norm(r0) / np.linalg.norm(r1))
            assert not np.isnan(ang[e])
            errs.append(abs(ang[e] - true))
    # 0.5 px of Gaussian noise per coordinate at a focal length of about 500 turns a ray by up to 0.5 * sqrt(2) / 500 rad = 0.08 degrees
    # (one sigma); the angle between two such rays moves by sqrt(2) of that, 0.115 degrees, and five sigma cover a few hundred matches
    assert len(errs) == s["n_right"][i] and max(errs) < np.deg2rad(5 * 0.115)
    # the other sign of the translation puts every midpoint behind the cameras
    assert np.isnan(MR.match_angles(s["norm05"], s["frame_off"], 2, 5, m[[e for e, r in enumerate(m.tolist()) if tuple(r) in right]], q, -t)).all()
    bad = np.array([[-1, 0], [0, 10 ** 6], [3, 3]])
    assert np.isnan(MR.match_angles(s["norm05"], s["frame_off"], 2, 5, bad, q, t)[:2]).all()


def test_seed_ties_relaxation_none():
    deg = np.deg2rad
    n_tri = np.array([900, 300, 250, 300, 400, 40, 500])
    angle = deg([0.1, 20.0, 30.0, 17.0, 9.0, 25.0, 40.0])
    ok = np.array([1, 1, 1, 1, 1, 1, 0])
    assert MR.seed(ok, n_tri, angle, 100, deg(16.0)) == 1 and MR.seed(ok, n_tri, angle, 100, deg(18.0)) == 1 and MR.seed(ok, n_tri, angle, 100, deg(21.0)) == 2
    assert MR.seed(ok, n_tri, angle, 50, deg(8.0)) == 4 and MR.seed(ok, n_tri, angle, 301, deg(8.0)) == 4 and MR.seed(ok, n_tri, angle, 401, deg(8.0)) == -1
    assert MR.seed(ok, n_tri, angle, 0, 0.0) == 0 and MR.seed(ok[:0], n_tri[:0], angle[:0], 0, 0.0) == -1
    assert MR.seed_relaxed(ok, n_tri, angle, 100, 16.0, 2) == (1, 0) and MR.seed_relaxed(ok, n_tri, angle, 100, 70.0, 2) == (1, 2)
    assert MR.seed_relaxed(ok, n_tri, angle, 100, 70.0, 1) == (-1, 1) and MR.seed_relaxed(ok, n_tri, angle, 1600, 16.0, 2) == (4, 2)


def test_correspond_against_sets():
    rng = np.random.RandomState(4)
    sizes = [30, 25, 0, 40, 35]
    fo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n, P = int(fo[-1]), 12
    row_frame = np.repeat(np.arange(5), sizes)
    for trial in range(5):
        registered = rng.uniform(size=5) < 0.5
        row_point = np.where(rng.uniform(size=n) < 0.8, rng.randint(0, P + 3, size=n), -1)      # some beyond the model
        edges = rng.randint(0, n, size=(900, 2))
        off, adj = MR.adjacency(n, edges)
        got = MR.correspond(off, adj, row_frame, fo, registered, row_point, P)
        want_rows, want_pts, drop = [], [], np.zeros(5, dtype=np.int64)
        for u in range(n):
            f = row_frame[u]
            if registered[f]:
                continue
            nb = [v for a, b in edges.tolist() for v in ((b,) if a == u and b != u else (a,) if b == u and a != u else ())]
            pts = [row_point[v] for v in nb if registered[row_frame[v]] and 0 <= row_point[v] < P]
            keep = sorted(set(pts))[:MR.MAX_LINKS]
            want_rows += [u] * len(keep); want_pts += keep
            drop[f] += sum(p not in keep for p in pts)
        assert got["corr_row"].tolist() == want_rows and got["corr_point"].tolist() == want_pts and got["dropped"].tolist() == drop.tolist()
        assert got["n_corr"].tolist() == np.bincount(row_frame[want_rows], minlength=5).tolist() if want_rows else not got["n_corr"].any()
        assert got["corr_off"].tolist() == np.concatenate([[0], np.cumsum(got["n_corr"])]).tolist()
        live = MR.live_edges(edges, row_frame, registered)
        assert all((r[0] >= 0) == bool(registered[row_frame[a]] and registered[row_frame[b]]) for r, (a, b) in zip(live.tolist(), edges.tolist()))


def test_choose_and_pack():
    n_corr, reg, tries = np.array([40, 0, 31, 40, 29, 30, 500]), np.array([0, 0, 0, 0, 0, 0, 1]), np.array([0, 0, 2, 1, 0, 3, 0])
    assert MR.choose(n_corr, reg, tries, 30, 3, 0)[0].tolist() == [0, 3, 2] and MR.choose(n_corr, reg, tries, 30, 3, 1)[1].tolist() == [40]
    assert MR.choose(n_corr, reg, tries, 30, 4, 0)[0].tolist() == [0, 3, 2, 5] and MR.choose(n_corr, reg, tries, 0, 9, 0)[0].tolist() == [0, 3, 2, 5, 4]
    corr = {"corr_off": np.array([0, 3, 3, 7]), "corr_row": np.arange(7), "corr_point": np.arange(7)[::-1]}
    kp, xyz = np.arange(14, dtype=np.float32).reshape(7, 2), np.arange(21, dtype=np.float64).reshape(7, 3)
    pk = MR.pack([2, 1, 0], corr, kp, xyz, 3)
    assert pk["counts"].tolist() == [3, 0, 3] and pk["cut"].tolist() == [1, 0, 0]
    assert pk["matched_keypoints"][0].tolist() == kp[3:6].tolist() and pk["matched_xyzs"][0].tolist() == xyz[[3, 2, 1]].tolist() and not pk["matched_xyzs"][1].any()


# ---------------------------------------------------------------- the host utilities
def test_umeyama_recovers_a_planted_similarity():
    from pram_amd.localization import mapper as MP
    rng = np.random.RandomState(2)
    for trial in range(20):
        src = rng.normal(size=(rng.randint(3, 40), 3)) * rng.uniform(0.1, 50.0)
        R, t, sc = PR.random_rotation(rng), rng.normal(size=3) * 10.0, rng.uniform(0.01, 100.0)
        s2, R2, t2 = MP.similarity_from_centres(src, sc * src @ R.T + t)
        assert abs(s2 / sc - 1.0) <= 1e-12 and np.abs(R2 - R).max() <= 1e-12 and np.abs(t2 - t).max() <= 1e-12 * max(1.0, np.abs(t).max(), sc * np.abs(src).max())
        assert abs(np.linalg.det(R2) - 1.0) <= 1e-12
    with pytest.raises(ValueError):
        MP.similarity_from_centres(src[:2], src[:2])
    with pytest.raises(ValueError):
        MP.similarity_from_centres(np.zeros((4, 3)), src[:4])


def test_apply_similarity_moves_poses_and_points_together():
    from pram_amd.localization import mapper as MP
    rng = np.random.RandomState(5)
    F, P = 6, 30
    Rs = [PR.random_rotation(rng) for _ in range(F)]
    res = {"qvecs": np.stack([PR.rot_to_qvec(R) for R in Rs]), "tvecs": rng.normal(size=(F, 3)), "point3D_xyzs": rng.normal(size=(P, 3)) + [0, 0, 6.0],
           "registered": np.array([1, 1, 1, 0, 1, 1], dtype=bool),
           "frames": [{"point3D_ids": np.array([1, -1, 3]), "xyzs": np.stack([rng.normal(size=3), np.zeros(3), rng.normal(size=3)])} for _ in range(F)]}
    res["qvecs"][3], res["tvecs"][3] = [1.0, 0.0, 0.0, 0.0], 0.0
    sc, R, t = 3.7, PR.random_rotation(rng), np.array([5.0, -2.0, 9.0])
    out = MP.apply_similarity(res, sc, R, t)
    X, Y = res["point3D_xyzs"], out["point3D_xyzs"]
    assert np.abs(Y - (sc * X @ R.T + t)).max() < 1e-12
    for f in (0, 1, 2, 4, 5):      # a point's camera coordinates scale by s, so its projection stays
        xc = X @ PR.qvec_to_rot(res["qvecs"][f]).T + res["tvecs"][f]
        yc = Y @ PR.qvec_to_rot(out["qvecs"][f]).T + out["tvecs"][f]
        assert np.abs(yc - sc * xc).max() < 1e-11 and out["qvecs"][f][0] >= 0
    assert np.array_equal(out["qvecs"][3], res["qvecs"][3]) and not out["tvecs"][3].any()
    assert not out["frames"][0]["xyzs"][1].any() and np.abs(out["frames"][0]["xyzs"][0] - (sc * R @ res["frames"][0]["xyzs"][0] + t)).max() < 1e-12
    assert np.abs(MP.centres(out["qvecs"], out["tvecs"])[0] - (sc * R @ MP.centres(res["qvecs"], res["tvecs"])[0] + t)).max() < 1e-11
    assert res["point3D_xyzs"] is X and not np.array_equal(out["tvecs"], res["tvecs"])      # the input is not modified


# ---------------------------------------------------------------- the header, the exports, the host logic on a stub
def test_header_and_exports(hip_lib):
    from pram_amd import _lib, ops
    # exported == declared, by type, and PRAM_MAP_MAX_LINKS == ops.MAP_MAX_LINKS: tests/test_abi_contract_cpu.py
    assert sorted(ENTRIES) == sorted(n for n in _lib.exported_symbols() if n.startswith("pram_map_"))
    assert MR.MAX_LINKS == ops.MAP_MAX_LINKS
    src = (ROOT / "pram_amd" / "csrc" / "mapper.hip").read_text()
    assert "atomicAdd" not in src and "while" not in src      # integer sums by shuffles, every loop bounded by an argument


def test_defaults_and_refusals_on_a_stub():
    from pram_amd._lib import PramHipError
    from pram_amd.localization import mapper as MP
    for k, v in MR.DEFAULTS.items():
        assert MP.MAP_DEFAULTS[k] == v, k
    assert MP.POSE_TRIALS == 1000 and MP.MAP_DEFAULTS["seed"] == 0 and MP.MAP_DEFAULTS["min_support"] == 0
    p = MP._map_params("t", {"twoview": {"trials": 64}, "bundle": {"cg_iters": 7}, "triangulation": {"trials": 9}})
    assert p["twoview"]["trials"] == 64 and p["twoview"]["pair_chunk"] == 256 and p["bundle"]["cg_iters"] == 7 and p["triangulation"]["trials"] == 9
    for bad in ({"min_cor": 3}, {"twoview": {"trails": 3}}, {"triangulation": {"min_support": 1}}, {"bundle": {"cg": 1}}):
        with pytest.raises(TypeError):
            MP._map_params("t", bad)
    for bad in ({"min_corr": -1}, {"max_rounds": 1.5}, {"max_corr": 3}, {"abs_pose_max_error": 0.0}, {"init_min_tri_angle": float("nan")},
                {"init_relax": 31}, {"bundle": {"max_iters": 3}}, {"bundle": {"frozen": [1]}}, {"bundle": {"cg_tol": 2.0}}, {"twoview": {"trials": 0}},
                {"abs_pose_min_inlier_ratio": -0.1}):
        with pytest.raises(ValueError):
            MP._map_params("t", bad)
    s = MR.rotation_scene()
    with pytest.raises(PramHipError):      # no CPU path
        MP.reconstruct(s["frames"], s["cameras"], s["pairs"], s["matches"], "cpu")
    with pytest.raises(TypeError):
        MP.reconstruct(s["frames"], s["cameras"], s["pairs"], s["matches"], "cpu", rounds=3)
    with pytest.raises(PramHipError):
        MP.choose_frames([1, 2], [0, 0], [0, 0], "cpu")
    empty = MP._empty_model(np.arange(3), np.array([0, 2, 2, 5]))
    assert len(empty["point_ids"]) == 0 and empty["point3D_xyzs"].shape == (0, 3) and empty["tracks"] == {} and len(empty["frames"]) == 3
    assert [f["point3D_ids"].tolist() for f in empty["frames"]] == [[-1, -1], [], [-1, -1, -1]]


# ---------------------------------------------------------------- the margins behind the GPU test's discrete comparisons
def test_margins_of_the_planted_scene():
    """Seed eligibility, n_corr against min_corr and the acceptance decide by thresholds; on the planted scene each holds with a
    margin that neither rounding nor the estimator's error can cross.  Measured with the planted relative poses and the planted
    matches: what the device estimates differs by the noise, a fraction of a degree and a few matches."""
    s = MR.planted_scene()
    d = MR.DEFAULTS
    rot = s["expected"]["rotation_pair"]
    assert len(s["matches"][rot]) == max(len(m) for m in s["matches"])
    eligible = []
    for i, (a, b) in enumerate(s["pairs"].tolist()):
        q, t = MR.true_relative(s, a, b)
        n, med = MR.lower_median(MR.match_angles(s["norm05"], s["frame_off"], a, b, s["matches"][i], q, t))
        med = float(np.degrees(med))
        assert abs(med - d["init_min_tri_angle"]) > 1.5, (a, b, med)                       # no pair within 1.5 degrees of the threshold
        assert abs(s["n_right"][i] - d["init_min_num_inliers"]) > 30 and abs(len(s["matches"][i]) - d["init_min_num_inliers"]) > 30
        if med > d["init_min_tri_angle"] and s["n_right"][i] > d["init_min_num_inliers"]:
            eligible.append(i)
    assert eligible and rot not in eligible and all(abs(a - b) == 3 and b < MR.N_MAIN for a, b in s["pairs"][eligible].tolist())
    q, t = MR.true_relative(s, 0, MR.F_ROT)
    # the rotation pair under ANY translation direction: the rays of a match are parallel up to the noise
    for t in (t, np.array([0.0, 1.0, 0.0]), np.array([0.6, 0.0, 0.8])):
        ang = MR.match_angles(s["norm05"], s["frame_off"], 0, MR.F_ROT, s["matches"][rot], q, t)
        assert np.degrees(np.nanmax(ang)) < 1.0 < d["init_min_tri_angle"] / 2 ** d["init_relax"]
    # n_corr: the rows of a frame matched (rightly) into a neighbour whose point two other main frames see as well
    seen = s["vis"][:MR.N_MAIN, :MR.N_POINTS]
    for f in list(range(MR.N_MAIN)) + [MR.F_ROT]:
        nb = [g for (a, b) in s["pairs"].tolist() for g in ((b,) if a == f else (a,) if b == f else ()) if g < MR.N_MAIN]
        can = sum(1 for pt in range(MR.N_POINTS) if (f, pt) in s["where"] and any((g, pt) in s["where"] for g in nb) and seen[:, pt].sum() >= 4)
        assert can >= 5 * d["min_corr"], (f, can)
    assert MR.N_FEW_SHARED <= d["min_corr"] // 3 and 0 < MR.N_FEW_SHARED      # at most ten rows of the few-frame lead to a point
    few = s["pairs"].tolist().index([s["few_partner"], MR.F_FEW])
    assert len(s["matches"][few]) == s["n_right"][few] >= 2 * 15              # enough for the two-view stage to keep the pair
    assert all(MR.F_FEW not in p and MR.F_ISO[0] not in p and MR.F_ISO[1] not in p for i, p in enumerate(s["pairs"].tolist()) if i < len(s["pairs"]) - 2)
    # the acceptance: four right matches in five, so the inlier share is far above 0.25 and the inliers far above 30
    share = s["n_right"][:-3] / np.array([len(m) for m in s["matches"][:-3]])
    assert share.min() > 0.75 > 2 * d["abs_pose_min_inlier_ratio"] and s["n_right"][:-3].min() > 5 * d["abs_pose_min_num_inliers"]
