"""GPU: statistical outlier removal on the device (pram_amd.localization.outliers, csrc/knn.hip) against the numpy restatement
tests/outliers_ref.py.  Everywhere: avg bit-equal, the statistics bit-equal, the mask and the inliers' indices equal; that follows
from the one fixed order of operations and from correctly rounded float64 sqrt and division (the library is built without
contraction).  tests/test_outliers_cpu.py checks the restatement itself and asserts the threshold's margin on every case here.
profiles/outliers_parity.md has the observed differences."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import outliers_ref as OR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def OL():
    from pram_amd.localization import outliers
    return outliers


_ran: dict = {}


def _device_run(OL, dev, name):
    if name not in _ran:
        xyz, k = OR.case(name)
        _ran[name] = OL.statistical_inliers(xyz, dev, nb_neighbors=k, std_ratio=2.0)
    return _ran[name]


def _bits(a):
    return np.asarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def _check(got: dict, want: dict, name: str):
    da = np.abs(got["avg_distance"] - want["avg_distance"])
    nb = int((_bits(got["avg_distance"]) != _bits(want["avg_distance"])).sum())
    print(f"{name}: avg differs in {nb} of {len(da)} entries (largest {da.max():.3e}); mean {got['mean']!r} / {want['mean']!r}, "
          f"std {got['std']!r} / {want['std']!r}, threshold {got['threshold']!r} / {want['threshold']!r}, n_valid {got['n_valid']}, "
          f"inliers {len(got['inlier_ids'])}")
    assert nb == 0
    assert np.array_equal(_bits([got[k] for k in ("mean", "std", "threshold")]), _bits([want[k] for k in ("mean", "std", "threshold")]))
    assert got["n_valid"] == want["n_valid"]
    assert got["mask"].dtype == np.bool_ and np.array_equal(got["mask"], want["mask"])
    assert got["inlier_ids"].dtype == np.int64 and np.array_equal(got["inlier_ids"], want["inlier_ids"])


@pytest.mark.parametrize("n", OR.SIZES)
def test_sizes(OL, dev, n):
    name = f"n_{n}"
    got, want = _device_run(OL, dev, name), OR.restated(name)
    _check(got, want, name)
    if n < 3:
        assert not got["mask"].any() and (np.isnan(got["threshold"]) or got["std"] == 0.0)


@pytest.mark.parametrize("k", OR.KS)
def test_list_sizes(OL, dev, k):
    name = f"k_{k}"
    got = _device_run(OL, dev, name)
    _check(got, OR.restated(name), name)
    if k == 1:      # the point itself is its nearest: avg = 0 everywhere, nothing is valid
        assert not got["avg_distance"].any() and got["n_valid"] == 0 and len(got["inlier_ids"]) == 0 and np.isnan(got["threshold"])


@pytest.mark.parametrize("name", ["planted_300", "planted_4000", "lattice", "offset", "big"])
def test_scenes(OL, dev, name):
    _check(_device_run(OL, dev, name), OR.restated(name), name)


def test_duplicates(OL, dev):
    xyz, far_dist, dup = OR.scene(1500, 4, 30, n_dup=24)
    got = _device_run(OL, dev, "dup25")
    _check(got, OR.restated("dup25"), "dup25")
    assert dup.sum() == 25 and not got["avg_distance"][dup].any() and not got["mask"][dup].any() and got["n_valid"] == 1500 - 25
    xyz, far_dist, dup = OR.planted(1500)      # five coincident points: valid, and in
    got = _device_run(OL, dev, "k_20")
    assert dup.sum() == 5 and (got["avg_distance"][dup] > 0).all() and got["mask"][dup].all()
    got = _device_run(OL, dev, "equal")
    _check(got, OR.restated("equal"), "equal")
    assert got["n_valid"] == 0 and not got["mask"].any() and len(got["inlier_ids"]) == 0 and np.isnan(got["mean"])


def test_permutation(OL, dev):
    perm = np.random.RandomState(OR.PERM_SEED).permutation(1500)
    a, b = _device_run(OL, dev, "k_20"), _device_run(OL, dev, "perm")
    _check(b, OR.restated("perm"), "perm")
    assert np.array_equal(_bits(b["avg_distance"]), _bits(a["avg_distance"][perm])) and np.array_equal(b["mask"], a["mask"][perm])
    ulp = np.spacing(a["threshold"])
    print(f"threshold {a['threshold']!r} / permuted {b['threshold']!r}: {abs(a['threshold'] - b['threshold']) / ulp:.1f} ulp")
    assert abs(a["threshold"] - b["threshold"]) <= 4 * ulp      # the sums follow the index


def test_two_runs_and_the_entries(OL, dev):
    from pram_amd import ops
    xyz, k = OR.case("n_3000")
    want = OR.restated("n_3000")
    a = _device_run(OL, dev, "n_3000")
    b = OL.statistical_inliers(torch.from_numpy(xyz).to(dev), dev)      # a device tensor, the defaults
    assert all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in a)
    avg = OL.knn_mean_distance(xyz, k, dev)
    assert avg.is_cuda and avg.dtype == torch.float64 and np.array_equal(_bits(avg.cpu().numpy()), _bits(want["avg_distance"]))
    sel = ops.sor_select(avg, 2.0)
    count = sel["count"].cpu().numpy()
    assert count.tolist() == [len(want["inlier_ids"]), want["n_valid"]] and sel["mask"].dtype == torch.uint8
    assert np.array_equal(sel["inlier_idx"][:count[0]].cpu().numpy(), want["inlier_ids"])
    stats = sel["stats"].cpu().numpy()
    assert np.array_equal(_bits(stats[:3]), _bits([want["mean"], want["std"], want["threshold"]])) and stats[3] == want["n_valid"]
    # another ratio moves the threshold only
    r1 = OL.statistical_inliers(xyz, dev, std_ratio=0.5)
    w1 = OR.select(want["avg_distance"], 0.5)
    assert r1["threshold"] == w1["threshold"] < a["threshold"] and np.array_equal(r1["mask"], w1["mask"]) and r1["mean"] == a["mean"]


def test_refusals_launch_nothing(OL, dev, hip_lib):
    from pram_amd import ops
    from pram_amd._lib import PramHipError
    L = hip_lib
    E_ARG = -1
    x = torch.from_numpy(OR.planted(300)[0]).to(dev)
    avg = torch.full((300,), -7.0, device=dev, dtype=torch.float64)
    ws = ops.sor_workspace(300, dev)
    stats = torch.full((4,), -7.0, device=dev, dtype=torch.float64)
    mask = torch.full((300,), 9, device=dev, dtype=torch.uint8)
    idx = torch.full((300,), -9, device=dev, dtype=torch.int32)
    count = torch.full((2,), -9, device=dev, dtype=torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    knn = lambda xp, n, k, ap: L.pram_knn_mean_distance(xp, n, k, ap, st)
    for args in ((p(x), 0, 20, p(avg)), (p(x), 2 ** 31, 20, p(avg)), (p(x), 300, 0, p(avg)), (p(x), 300, ops.KNN_MAX_K + 1, p(avg)),
                 (None, 300, 20, p(avg)), (p(x), 300, 20, None), (p(x) + 4, 299, 20, p(avg)), (p(x), 300, 20, p(avg) + 4)):
        assert knn(*args) == E_ARG, args
    assert knn(p(x), 300, ops.KNN_MAX_K + 1, p(avg)) == E_ARG and b"PRAM_KNN_MAX_K" in L.pram_last_error()
    sel = lambda ap, n, ratio, wp, wb, sp, mp, ip, cp: L.pram_sor_select(ap, n, C.c_double(ratio), wp, wb, sp, mp, ip, cp, st)
    good = (p(avg), 300, 2.0, p(ws), ws.numel(), p(stats), p(mask), p(idx), p(count))
    for at, bad in ((1, 0), (1, 2 ** 31), (2, 0.0), (2, -1.0), (2, float("nan")), (4, ws.numel() - 1), (0, None), (3, None), (5, None), (6, None),
                    (7, None), (8, None), (0, p(avg) + 4), (3, p(ws) + 4), (5, p(stats) + 4), (7, p(idx) + 2), (8, p(count) + 2)):
        args = list(good)
        args[at] = bad
        assert sel(*args) == E_ARG, (at, bad)
    torch.cuda.synchronize()
    assert (avg == -7.0).all() and (stats == -7.0).all() and (mask == 9).all() and (idx == -9).all() and (count == -9).all()
    assert ops.sor_workspace(300, dev).numel() >= 12
    with pytest.raises(PramHipError):
        ops.sor_workspace(0, dev)
    for bad in (33, 64):
        with pytest.raises((ValueError, PramHipError), match="PRAM_KNN_MAX_K"):
            OL.statistical_inliers(OR.planted(300)[0], dev, nb_neighbors=bad)
    with pytest.raises(PramHipError, match="PRAM_KNN_MAX_K"):
        ops.knn_mean_distance(x, 33)
    for bad in (np.zeros((4, 2)), np.zeros((0, 3)), np.array([[0.0, np.inf, 0.0]]), np.array([[0.0, np.nan, 0.0]])):
        with pytest.raises(ValueError):
            OL.statistical_inliers(bad, dev)
    with pytest.raises(ValueError):
        OL.statistical_inliers(torch.tensor([[0.0, float("nan"), 0.0]], dtype=torch.float64, device=dev), dev)
    with pytest.raises(ValueError):
        OL.statistical_inliers(torch.zeros(4, 3, device=dev), dev)      # float32


def test_end_to_end_after_triangulation(OL, dev):
    """triangulate_map -> far points appended to the model's tables (tracks that wrong matches made consistent: each seen by two
    frames) -> remove_statistical_outliers -> label_points -> landmarks_from_labels -> build_store_inputs -> ReferenceStore."""
    from pram_amd.localization import labelling as LB
    from pram_amd.localization import mapbuild as MB
    from pram_amd.localization import triangulation as TG
    from pram_amd.localization.candidates import ReferenceStore
    from tests import pose_ref as PR
    from tests import triangulation_ref as TR
    s = TR.tri_scene()
    m = TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev)
    # the planted far points take the keypoints of frames 0 and 1 that have no point
    rng = np.random.RandomState(21)
    n_far = 6
    free = [np.nonzero(m["frames"][f]["point3D_ids"] < 0)[0] for f in (0, 1)]
    assert min(len(free[0]), len(free[1])) >= n_far
    far_ids = np.arange(n_far, dtype=np.int64) + int(m["point_ids"].max()) + 1
    d = rng.normal(size=(n_far, 3))
    far_xyz = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(60.0, 200.0, size=(n_far, 1))
    model = dict(m)
    model["point_ids"] = np.concatenate([m["point_ids"], far_ids])
    model["point3D_xyzs"] = np.concatenate([m["point3D_xyzs"], far_xyz])
    model["track_error"] = np.concatenate([m["track_error"], np.ones(n_far)])
    model["tracks"], model["point3D_frame_ids"] = dict(m["tracks"]), dict(m["point3D_frame_ids"])
    model["frames"] = [{k: v.copy() for k, v in f.items()} for f in m["frames"]]
    for j, pid in enumerate(far_ids.tolist()):
        kp = (int(free[0][j]), int(free[1][j]))
        model["tracks"][pid] = (np.array([0, 1]), np.array(kp, dtype=np.int64))
        model["point3D_frame_ids"][pid] = np.array([0, 1])
        for f in (0, 1):
            model["frames"][f]["point3D_ids"][kp[f]], model["frames"][f]["xyzs"][kp[f]] = pid, far_xyz[j]
    want = OR.statistical_inliers(model["point3D_xyzs"], 20, 2.0)
    assert not want["mask"][-n_far:].any() and OR.margin(want) > 1e-9
    out = OL.remove_statistical_outliers(model, dev)
    kept = ~np.isin(model["point_ids"], out["removed_ids"])
    _check({**out, "mask": kept, "inlier_ids": np.nonzero(kept)[0].astype(np.int64)}, want, "end to end")
    gone = set(out["removed_ids"].tolist())
    assert set(far_ids.tolist()) <= gone and np.array_equal(out["point_ids"], model["point_ids"][want["mask"]])
    assert not gone & set(out["point_ids"].tolist()) and not gone & set(out["tracks"]) and not gone & set(out["point3D_frame_ids"])
    assert all(not np.isin(f["point3D_ids"], out["removed_ids"]).any() for f in out["frames"])
    assert all((f["point3D_ids"] >= 0).sum() < (g["point3D_ids"] >= 0).sum() for f, g in zip(out["frames"][:2], model["frames"][:2]))
    assert len(model["point_ids"]) == len(m["point_ids"]) + n_far and set(far_ids.tolist()) <= set(model["tracks"])      # the input stands
    # the chain goes on exactly as after triangulate_map
    xyz = dict(zip(out["point_ids"].tolist(), out["point3D_xyzs"]))
    lab = LB.label_points(out["tracks"], xyz, 4, dev, min_obs=2)
    keep_ids = model["point_ids"][want["mask"]]
    ref_xyz = dict(zip(keep_ids.tolist(), model["point3D_xyzs"][want["mask"]]))
    ref_lab = LB.label_points({p: model["tracks"][p] for p in model["tracks"] if p in ref_xyz}, ref_xyz, 4, dev, min_obs=2)
    assert np.array_equal(lab["id"], ref_lab["id"]) and np.array_equal(lab["label"], ref_lab["label"]) and np.array_equal(lab["id"], keep_ids)
    landmarks, sids = LB.landmarks_from_labels(lab["id"], lab["label"])
    rng = np.random.RandomState(9)
    frames = []
    for f in range(s["n_frames"]):
        kp = s["frames"][f]["keypoints"]
        dsc = rng.normal(size=(len(kp), 128)).astype(np.float32)
        pid = out["frames"][f]["point3D_ids"]
        fx, fy, cx, cy = PR.unify(int(s["cam_model"][f]), s["cam_params"][f])[:4]
        frames.append({"keypoints": np.concatenate([kp, np.ones((len(kp), 1), dtype=np.float32)], 1), "descriptors": dsc / np.linalg.norm(dsc, axis=1, keepdims=True),
                       "xyzs": out["frames"][f]["xyzs"], "point3D_ids": pid, "keypoint_segs": np.array([sids.get(int(p), 0) for p in pid], dtype=np.int32),
                       "width": TR.WIDTH, "height": TR.HEIGHT, "qvec": s["qvec"][f], "tvec": s["tvec"][f], "intrinsics": (fx, fy, cx, cy)})
    built = MB.build_store_inputs(frames, out["tracks"], landmarks, xyz, dev, min_obs=2, n_vrf=3)
    store = ReferenceStore(frames, point3D_sids=sids, **{k: built[k] for k in MB.STORE_KEYS})
    assert np.array_equal(store.pt_ids, out["point_ids"]) and np.array_equal(store._point_values()["pt_xyz"], out["point3D_xyzs"])
    assert not np.isin(store.point3D_ids, out["removed_ids"]).any()
