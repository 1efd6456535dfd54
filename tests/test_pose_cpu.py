"""The numpy restatement of the pose stage (tests/pose_ref.py) against itself and against scipy, so that the yardstick of
tests/test_gpu_pose.py is trusted before the device is compared with it; plus the host-side pieces of the feature."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pose_ref as pr      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pram_pose_prepare", "pram_pose_hypotheses", "pram_pose_score", "pram_pose_refine", "pram_pose_select")
# bars of the scipy comparison (profiles/pose_parity.md: ten times the largest figure measured with this file: 2.4e-4 degrees and
# 1.3e-5 m, both on the 8-inlier scene, where 2 x 20 LM iterations stop 8e-7 above BFGS's cost)
SCIPY_ROT_DEG = 2.5e-3
SCIPY_CENTRE_M = 1.3e-4
P3P_SEEDS = (1, 2, 3)
P3P_COND = 1e-6              # a trial whose best-conditioned.. worst root has |f'(v) v| / sum |A_i v^i| below this is near-degenerate


@pytest.mark.parametrize("name", list(pr.SCENE_CAMERAS))
def test_distort_undistort_round_trip(name):
    model, params = pr.camera_row(pr.SCENE_CAMERAS[name])
    c = pr.unify(model, params)
    rng = np.random.default_rng(0)
    u, v = rng.uniform(-0.6, 0.6, 500), rng.uniform(-0.4, 0.4, 500)
    ud, vd = pr.distort(u, v, *c[4:])
    u2, v2 = pr.undistort(ud, vd, *c[4:])
    assert max(np.abs(u2 - u).max(), np.abs(v2 - v).max()) < 1e-13
    # and through prepare: pixels -> plane
    px = np.stack([c[0] * ud + c[2], c[1] * vd + c[3]], 1)
    pts = pr.prepare((px - 0.5).astype(np.float32), model, params)
    assert np.abs(pts - np.stack([u, v], 1)).max() < 2e-4 / min(c[0], c[1])      # float32 pixels: 2^-14 px at 1000 px


def test_sampler_distinct_and_in_range():
    for n in (3, 4, 5, 17, 2048):
        tri = pr.sample_triples(5, 2, n, 4000)
        assert tri.min() >= 0 and tri.max() < n
        assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 0] != tri[:, 2]).all() and (tri[:, 1] != tri[:, 2]).all()
        if n <= 5:      # every row is drawn
            assert set(np.unique(tri)) == set(range(n))
    assert pr.sm64(np.array([0], dtype=np.uint64))[0] == np.uint64(0xE220A8397B1DCDAF)      # splitmix64's first output for seed 0


@pytest.mark.parametrize("name", list(pr.SCENE_CAMERAS))
def test_p3p_noise_free(name):
    cam = pr.SCENE_CAMERAS[name]
    s = pr.make_scene(3, cam, 400, 0.0, noise_px=0.0)
    model, params = pr.camera_row(cam)
    c = pr.unify(model, params)
    px, _ = pr.project(s["xyz"], s["R"], s["t"], model, params)
    u, v = pr.undistort((px[:, 0] - c[2]) / c[0], (px[:, 1] - c[3]) / c[1], *c[4:])
    pts = np.stack([u, v], 1)
    tri = pr.sample_triples(1, 0, 400, 300)
    poses, ns, cond = pr.p3p(pts[tri], s["xyz"][tri], True)
    gt = np.concatenate([s["R"], s["t"][:, None]], 1).reshape(12)
    well = cond > 1e-4
    assert well.mean() > 0.9
    for h in np.nonzero(well)[0]:
        assert ns[h] >= 1
        assert np.abs(poses[h, :ns[h]] - gt).max(1).min() < 1e-5 * (1.0 + np.abs(s["t"]).max()), h
        for k in range(ns[h]):      # every root reprojects its three points, all in front
            R, t = pr.pose_12(poses[h, k])
            xc = s["xyz"][tri[h]] @ R.T + t
            assert (xc[:, 2] > 0).all()
            assert np.abs(xc[:, :2] / xc[:, 2:] - pts[tri[h]]).max() < 1e-7
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.linalg.det(R) > 0.999


def test_p3p_near_degenerate_share():
    """The seeds test_gpu_pose.py compares root for root leave out fewer than 1 % of the trials."""
    s = pr.make_scene(11, pr.SCENE_CAMERAS["OPENCV"], 500, 0.3)
    model, params = pr.camera_row(s["cam"])
    pts = pr.prepare(s["kpts"], model, params)
    for seed in P3P_SEEDS:
        _, _, cond = pr.hypotheses(pts, s["xyz"], seed, 0, 1000, True)
        assert (cond < P3P_COND).mean() < 0.01, seed


def test_degenerate_triples_give_no_solution():
    x = np.array([[[0.0, 0.0], [0.1, 0.0], [0.2, 0.1]]])
    line = np.array([[[0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [2.0, 0.0, 5.0]]])
    dup = np.array([[[0.0, 0.0, 5.0], [0.0, 0.0, 5.0], [2.0, 1.0, 5.0]]])
    for X in (line, dup):
        poses, ns = pr.p3p(x, X)
        assert ns[0] == 0 and not np.any(poses) and np.all(np.isfinite(poses))


@pytest.fixture(scope="module")
def e2e():
    scenes = pr.e2e_scenes()
    return scenes, [pr.estimate_pose(s["kpts"], s["xyz"], s["cam"], threshold=pr.E2E_THRESHOLD, refine_iters=20, seed=7, p=i)
                    for i, s in enumerate(scenes)]


def test_restatement_recovers_the_planted_pose(e2e):
    """1 px noise is atan(1 / 500) = 0.11 degrees per point at the shortest focal length; with 8 or more inliers the pose is good
    to a few times that: 1 degree and (30 m deepest point x 1 degree) 0.5 m are generous and fixed."""
    for s, r in zip(*e2e):
        assert r["success"] and r["refined"]
        er, ec = pr.pose_errors(r["R"], r["tvec"], s["R"], s["t"])
        print(s["cam"][0], s["n"], r["num_inliers"], er, ec)
        assert er < 1.0 and ec < 0.5
        assert r["num_inliers"] >= 0.9 * (~s["outlier"]).sum()
        assert abs(np.linalg.norm(r["qvec"]) - 1.0) < 1e-12 and r["qvec"][0] >= 0
        assert np.abs(pr.qvec_to_rot(r["qvec"]) - r["R"]).max() < 1e-9


def test_restatement_agrees_with_scipy(e2e):
    """Against an independent minimiser (BFGS) of the same per-point Cauchy cost, started from the planted pose."""
    for s, r in zip(*e2e):
        Rs, ts = pr.scipy_refine(s, r["inliers"], s["R"], s["t"])
        er, ec = pr.pose_errors(r["R"], r["tvec"], Rs, ts)
        print(s["cam"][0], s["n"], r["num_inliers"], "rot", er, "deg; centre", ec, "m")
        assert er < SCIPY_ROT_DEG and ec < SCIPY_CENTRE_M


def test_restatement_failures():
    cam = pr.SCENE_CAMERAS["PINHOLE"]
    s = pr.make_scene(1, cam, 50, 0.0)
    for n in (0, 1, 2):
        r = pr.estimate_pose(s["kpts"][:n], s["xyz"][:n], cam, threshold=4.0, trials=50)
        assert not r["success"] and r["num_inliers"] == 0 and r["inliers"].shape == (n,)
    behind = s["xyz"] - 2.0 * (s["xyz"] + s["R"].T @ s["t"])      # mirrored through the camera centre: every depth negative
    # any non-degenerate triple supports its own P3P roots, so "no pose" is a matter of min_inlier_ratio: 3 rows of 50 pass 0.01
    r = pr.estimate_pose(s["kpts"], behind, cam, threshold=4.0, trials=200, min_inlier_ratio=0.3)
    assert not r["success"] and r["n0"] < 15 and r["num_inliers"] == 0 and not r["inliers"].any()


def test_select_rule():
    assert pr.select([1, 1, 1], [10, 50, 70], 40) == (1, 1, 1)          # the first over min_inliers wins
    assert pr.select([1, 1, 1], [10, 30, 30], 40) == (1, 0, 1)          # none over: the first with strictly most
    assert pr.select([0, 0], [0, 0], 40) == (-1, -1, -1)
    assert pr.select([0, 1, 1], [0, 50, 90], 40) == (1, 1, 1)
    assert pr.select([1, 0, 1], [20, 0, 45], 40) == (2, 1, 2)


def test_camera_table():
    from pram_amd.localization.pose import camera_table
    ids, params = camera_table(list(pr.SCENE_CAMERAS.values()))
    assert ids.dtype == np.int32 and params.dtype == np.float64 and params.shape == (5, 8)
    for i, cam in enumerate(pr.SCENE_CAMERAS.values()):
        m, p = pr.camera_row(cam)
        assert ids[i] == m and np.array_equal(params[i], p)
    with pytest.raises(ValueError):
        camera_table([("FULL_OPENCV", 640, 480, [1.0] * 12)])
    with pytest.raises(ValueError):
        camera_table([("RADIAL", 640, 480, [500.0, 320.0, 240.0])])


def test_exported_symbols():
    from pram_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "pram_hip.h")).read()
    # the entries' declarations and the types of their ctypes signatures: tests/test_abi_contract_cpu.py
    assert set(ENTRIES) <= set(_lib.exported_symbols()) and all(_lib._SIGS[name][0] is _lib.I for name in ENTRIES)
    for fn in ("pose_prepare", "pose_hypotheses", "pose_score", "pose_refine", "pose_select"):
        assert callable(getattr(ops, fn))
    for k, v in pr.MODELS.items():
        assert ops.CAMERA_MODELS[k] == v and re.search(r"#define PRAM_CAM_%s %d\b" % (k, v), header)


def test_camera_form():
    """The three forms of a ``cameras`` argument, and that a malformed tuple counts as camera tuples (camera_table rejects it)."""
    import torch
    from pram_amd.localization.pose import camera_form, camera_table, device_cameras
    cams = list(pr.SCENE_CAMERAS.values())
    table = camera_table(cams)
    assert camera_form(cams) == "tuples" and camera_form(tuple(cams)) == "tuples" and camera_form([]) == "tuples"
    assert camera_form(table) == "table"
    resident = device_cameras(table, "cpu")
    assert camera_form(resident) == "resident" and camera_form(device_cameras(cams, "cpu")) == "resident"
    assert torch.equal(resident[0], torch.from_numpy(table[0])) and resident[2] == table[0].tolist()
    # two lists are no camera_table result, three arrays no device_cameras result: both go to camera_table, which refuses them
    for bad in ((table[0].tolist(), table[1].tolist()), (table[0], table[1], table[0].tolist())):
        assert camera_form(bad) == "tuples"
        with pytest.raises((ValueError, IndexError, TypeError)):
            device_cameras(bad, "cpu")


def test_read_back_round_trips():
    """ReadBack on CPU tensors: qvec / tvec bit for bit, the int32 values -1, 0 and 2**31 - 1 through float64, a ragged tail cut to
    its count, and the second block behind the rows."""
    import torch
    from pram_amd.localization.pose import ReadBack
    rng = np.random.default_rng(5)
    P, k = 6, 4
    q, t = rng.standard_normal((P, 4)), rng.standard_normal((P, 3)) * 1e3
    q[0, 0], t[1, 2], q[2, 1] = np.nextafter(1.0, 2.0), -0.0, 5e-324      # one ulp above 1, a negative zero, a subnormal
    est = {"qvec": torch.from_numpy(q), "tvec": torch.from_numpy(t)}
    a = np.array([-1, 0, 2 ** 31 - 1, 7, -2 ** 31, 1], dtype=np.int32)
    n_tail = np.array([0, 1, 4, 2, 3, 4], dtype=np.int32)
    tail = rng.integers(0, 2 ** 31 - 1, (P, k)).astype(np.int32)
    block = rng.integers(-1, 2 ** 31 - 1, (3, 3)).astype(np.int32)
    ints = {"first": torch.from_numpy(a), "n_tail": torch.from_numpy(n_tail), "last": torch.from_numpy(a[::-1].copy())}
    rb = ReadBack(est, ints, tail=torch.from_numpy(tail), tail_count="n_tail", block=torch.from_numpy(block))
    assert len(rb) == P and rb.block.dtype == np.int64 and np.array_equal(rb.block, block)
    for i in range(P):
        v = rb[i]
        assert v["qvec"].tobytes() == q[i].tobytes() and v["tvec"].tobytes() == t[i].tobytes()
        assert (v["first"], v["n_tail"], v["last"]) == (int(a[i]), int(n_tail[i]), int(a[P - 1 - i])) and type(v["first"]) is int
        assert v["tail"].tolist() == tail[i, :n_tail[i]].tolist()
        v["qvec"][0] = 0.0      # a copy: the next look is unchanged
        assert rb[i]["qvec"].tobytes() == q[i].tobytes()
    plain = ReadBack(est, {"only": torch.from_numpy(a)})
    assert plain.block is None and set(plain[2]) == {"qvec", "tvec", "only"} and plain[2]["only"] == 2 ** 31 - 1
    empty = ReadBack({"qvec": torch.zeros(0, 4, dtype=torch.float64), "tvec": torch.zeros(0, 3, dtype=torch.float64)},
                     {"only": torch.zeros(0, dtype=torch.int32)}, block=torch.zeros(0, 3, dtype=torch.int32))
    assert len(empty) == 0 and empty.block.shape == (0, 3)
