"""CPU: the numpy restatement of the statistical outlier removal (tests/outliers_ref.py) against an independent implementation
(scipy's k-d tree, the row mean, numpy's std(ddof=1)), its edge rules, the margins that make the device's mask exact on every
case tests/test_gpu_outliers.py runs, and the host side of pram_amd.localization.outliers that needs no GPU.

Nothing here is pinned to Open3D, which is not installed: the restatement is Open3D's algorithm as include/pram_hip.h states it.

The bar on avg.  The k-d tree returns sqrt of a sum of squares added in another order and numpy's mean adds the row pairwise: a
few ulp of a distance, which is below 2 * sqrt(3) * max|coordinate|.  1e-12 * max|coordinate| is three orders above the 5.7e-14
measured at coordinates up to 320."""
from pathlib import Path

import numpy as np
import pytest

from tests import outliers_ref as OR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_knn_mean_distance", "pram_sor_workspace_bytes", "pram_sor_select")


def test_symbols_declared_and_exported(hip_lib):
    # the entries' declarations, types and exports and header == ops for KNN_TILE, KNN_MAX_K and SOR_BLOCK: tests/test_abi_contract_cpu.py
    from pram_amd import _lib, ops
    header = (ROOT / "include" / "pram_hip.h").read_text()
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    assert OR.BLOCK == ops.SOR_BLOCK and OR.MAX_K == ops.KNN_MAX_K == 32 and "PRAM_KNN_MAX_K" in header.split("#ifndef PRAM_HIP_H")[0]
    assert (ROOT / "pram_amd" / "csrc" / "knn.hip").exists()
    L = hip_lib
    assert L.pram_sor_workspace_bytes(5000) >= 5 * (8 + 4)
    for n in (0, -1, 2 ** 31):
        assert L.pram_sor_workspace_bytes(n) == 0, n


@pytest.mark.parametrize("n", list(OR.SCENES))
def test_restatement_equals_a_kd_tree(n):
    from scipy.spatial import cKDTree
    xyz, far_dist, dup = OR.planted(n)
    r = OR.restated("k_20" if n == 1500 else f"planted_{n}")
    d, _ = cKDTree(xyz).query(xyz, 20)
    avg = d.mean(axis=1)
    valid = avg > 0
    threshold = avg[valid].mean() + 2.0 * avg[valid].std(ddof=1)
    mask = valid & (avg < threshold)
    dev = float(np.abs(avg - r["avg_distance"]).max())
    print(f"n = {n}: largest |avg - avg_kdtree| {dev:.3e} at coordinates up to {np.abs(xyz).max():.0f}, mask differences {int((mask != r['mask']).sum())}")
    assert np.array_equal(mask, r["mask"]) and np.array_equal(np.nonzero(mask)[0], r["inlier_ids"])
    assert dev <= 1e-12 * np.abs(xyz).max()
    assert r["n_valid"] == n and abs(r["threshold"] - threshold) <= 1e-12 * threshold
    # what the filter is for: the planted points far out are gone, the clusters stay, and so does the group of five coincident points
    far, sure = far_dist > 0, far_dist >= OR.SURE
    out = ~r["mask"]
    print(f"n = {n}: {int(out[far].sum())} of {int(far.sum())} planted points out ({int(sure.sum())} of them beyond {OR.SURE:.0f} m), "
          f"{int(out[~far].sum())} of {int((~far).sum())} cluster points out")
    assert sure.sum() >= 3 and out[sure].all()
    assert out[~far].sum() <= 0.05 * (~far).sum()
    assert dup.sum() == OR.N_DUP + 1 and r["mask"][dup].all() and len(np.unique(xyz[dup], axis=0)) == 1


@pytest.mark.parametrize("name", OR.CASES)
def test_margin_of_every_gpu_case(name):
    """The device's statistics equal the restatement's bit for bit, so its mask does too; the margin says that the mask would
    survive a threshold that differed in its last bits (the permuted case's may, by 4 ulp).  Cases without a spread have no
    threshold to be near: their mask is all zero by rule."""
    r = OR.restated(name)
    if r["n_valid"] < 2 or not r["std"] > 0:
        assert name in ("n_1", "n_2", "k_1", "equal") and not r["mask"].any()
        return
    m = OR.margin(r)
    print(f"{name}: margin {m:.3e}")
    assert m > 1e-9


def test_edge_rules():
    rs = np.random.RandomState(5)
    x = rs.normal(0.0, 3.0, size=(60, 3))
    # n < k: every point's list is the whole cloud
    r = OR.statistical_inliers(x[:7], 20, 2.0)
    want = np.array([np.sqrt(((x[:7] - p) ** 2).sum(1)).sum() / 7 for p in x[:7]])
    assert np.abs(r["avg_distance"] - want).max() <= 1e-13 and r["n_valid"] == 7
    # k coincident points: each has k - 1 duplicates, avg = 0, not valid, out; k - 1 of them: valid
    k = 6
    for copies, valid in ((k, False), (k - 1, True)):
        y = np.concatenate([x, np.repeat(x[:1] + 50.0, copies, axis=0)])
        r = OR.statistical_inliers(y, k, 2.0)
        grp = np.arange(len(y)) >= 60
        assert ((r["avg_distance"][grp] > 0) == valid).all() and r["n_valid"] == 60 + (copies if valid else 0)
        assert not r["mask"][grp].any() or valid
    # all points equal: nothing valid, no threshold, no inliers
    r = OR.statistical_inliers(np.full((30, 3), 1.5), 20, 2.0)
    assert r["n_valid"] == 0 and not r["mask"].any() and np.isnan(r["threshold"]) and np.isnan(r["std"]) and np.isnan(r["mean"])
    # one valid point: k = 2, two pairs of coincident points and one point alone
    y = np.array([[0, 0, 0], [0, 0, 0], [9, 9, 9], [1, 0, 0], [1, 0, 0]], dtype=np.float64)
    r = OR.statistical_inliers(y, 2, 2.0)
    assert r["n_valid"] == 1 and r["mean"] == r["avg_distance"][2] > 0 and np.isnan(r["threshold"]) and not r["mask"].any() and len(r["inlier_ids"]) == 0
    # strict: two points, equal avg, std 0, threshold == avg: out
    r = OR.statistical_inliers(np.array([[0.0, 0, 0], [3.0, 4.0, 0]]), 20, 2.0)
    assert r["avg_distance"].tolist() == [2.5, 2.5] and r["std"] == 0.0 and r["threshold"] == 2.5 and not r["mask"].any()
    for bad in ((0, 2.0), (20, 0.0), (20, -1.0), (20, float("nan"))):
        with pytest.raises(ValueError):
            OR.statistical_inliers(x, *bad)


def test_blocked_sums_follow_the_block():
    v = np.random.RandomState(3).uniform(0.0, 1.0, size=2 * OR.BLOCK + 17)
    ok = np.random.RandomState(4).uniform(size=v.shape) < 0.9
    acc = 0.0
    for b in range(3):
        s = 0.0
        for t in v[b * OR.BLOCK:(b + 1) * OR.BLOCK][ok[b * OR.BLOCK:(b + 1) * OR.BLOCK]]:
            s = s + t
        acc = acc + s
    assert OR.blocked_sum(v, ok) == acc and abs(acc - v[ok].sum()) <= 1e-12 * acc


# ---------------------------------------------------------------- the host side, with the inlier set injected
def _model():
    ids = np.array([3, 4, 7, 9, 12, 20], dtype=np.int64)
    xyz = np.arange(18, dtype=np.float64).reshape(6, 3) + 1.0
    tracks = {int(p): (np.array([0, 1 + i % 2]), np.array([i, i + 1])) for i, p in enumerate(ids)}
    frames = [{"point3D_ids": np.array([3, -1, 7, 12, 20], dtype=np.int64), "xyzs": np.ones((5, 3)), "name": "a"},
              {"point3D_ids": np.array([4, 9, 9, -1], dtype=np.int64), "xyzs": np.full((4, 3), 2.0)},
              {"point3D_ids": np.zeros(0, dtype=np.int64), "xyzs": np.zeros((0, 3))}]
    return {"point_ids": ids, "point3D_xyzs": xyz, "track_error": np.arange(6) * 0.5, "tracks": tracks,
            "point3D_frame_ids": {p: t[0] for p, t in tracks.items()}, "frames": frames, "pair_index": np.arange(4), "inlier_ratio": np.ones(4)}


def _inject(monkeypatch, keep, seen):
    from pram_amd.localization import outliers as OL
    keep = np.asarray(keep, dtype=bool)

    def fake(xyz, device, nb_neighbors=20, std_ratio=2.0):
        seen.update(xyz=np.array(xyz), device=device, k=nb_neighbors, ratio=std_ratio)
        return {"inlier_ids": np.nonzero(keep)[0], "mask": keep, "avg_distance": np.arange(len(keep)) + 0.25, "mean": 1.0, "std": 2.0,
                "threshold": 5.0, "n_valid": len(keep)}

    monkeypatch.setattr(OL, "statistical_inliers", fake)
    return OL


def _frozen(a):
    import copy
    return copy.deepcopy(a)


def _same(a, b) -> bool:
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_remove_statistical_outliers_bookkeeping(monkeypatch):
    seen = {}
    OL = _inject(monkeypatch, [1, 0, 1, 0, 1, 1], seen)
    m = _model()
    before = _frozen(m)
    out = OL.remove_statistical_outliers(m, "cuda:0", nb_neighbors=7, std_ratio=1.5)
    assert _same(m, before)      # the input is untouched
    assert np.array_equal(seen["xyz"], m["point3D_xyzs"]) and (seen["k"], seen["ratio"], seen["device"]) == (7, 1.5, "cuda:0")
    assert out["point_ids"].tolist() == [3, 7, 12, 20] and out["removed_ids"].tolist() == [4, 9]      # ids kept, order preserved
    assert np.array_equal(out["point3D_xyzs"], m["point3D_xyzs"][[0, 2, 4, 5]]) and out["track_error"].tolist() == [0.0, 1.0, 2.0, 2.5]
    assert list(out["tracks"]) == [3, 7, 12, 20] == list(out["point3D_frame_ids"])
    assert all(out["tracks"][p] is m["tracks"][p] for p in out["tracks"])
    f0, f1, f2 = out["frames"]
    assert f0["point3D_ids"].tolist() == [3, -1, 7, 12, 20] and np.array_equal(f0["xyzs"], np.ones((5, 3))) and f0["name"] == "a"
    assert f1["point3D_ids"].tolist() == [-1, -1, -1, -1] and f1["point3D_ids"].dtype == np.int64
    assert not f1["xyzs"][:3].any() and f1["xyzs"][3].tolist() == [2.0, 2.0, 2.0]      # a keypoint that had no point keeps what it had
    assert f2["point3D_ids"].shape == (0,) and f2["xyzs"].shape == (0, 3)
    assert out["pair_index"] is m["pair_index"] and out["inlier_ratio"] is m["inlier_ratio"]      # every other key passes through
    assert (out["mean"], out["std"], out["threshold"], out["n_valid"]) == (1.0, 2.0, 5.0, 6) and out["avg_distance"].shape == (6,)
    assert set(out) == set(m) | {"removed_ids", "avg_distance", "mean", "std", "threshold", "n_valid"}


def test_filter_points_bookkeeping(monkeypatch):
    seen = {}
    OL = _inject(monkeypatch, [0, 1, 1, 1, 0, 1], seen)
    m = _model()
    xyzs = {int(p): m["point3D_xyzs"][i] for i, p in reversed(list(enumerate(m["point_ids"])))}      # the cloud follows the dict's order
    tracks = dict(m["tracks"])
    tracks[99] = (np.array([0]), np.array([0]))      # a track without xyz is none of this step's business
    t0, x0 = dict(tracks), dict(xyzs)
    t, x, info = OL.filter_points(tracks, xyzs, "cuda:0")
    assert np.array_equal(seen["xyz"], m["point3D_xyzs"][::-1]) and (seen["k"], seen["ratio"]) == (20, 2.0)
    assert info["removed_ids"].tolist() == [20, 4] and list(x) == [12, 9, 7, 3] and list(t) == [3, 7, 9, 12, 99]
    assert all(x[p] is xyzs[p] for p in x) and all(t[p] is tracks[p] for p in t)
    assert list(tracks) == list(t0) and list(xyzs) == list(x0)
    assert set(info) == {"removed_ids", "avg_distance", "mean", "std", "threshold", "n_valid"}


def test_refusals_before_any_device():
    from pram_amd._lib import PramHipError
    from pram_amd.localization import outliers as OL
    x = OR.planted(300)[0]
    with pytest.raises(PramHipError):
        OL.statistical_inliers(x, "cpu")
    with pytest.raises(ValueError, match="PRAM_KNN_MAX_K"):
        OL.statistical_inliers(x, "cuda:0", nb_neighbors=33)
    for kw in (dict(nb_neighbors=0), dict(std_ratio=0.0), dict(std_ratio=float("nan"))):
        with pytest.raises(ValueError):
            OL.statistical_inliers(x, "cuda:0", **kw)
    with pytest.raises(ValueError, match="PRAM_KNN_MAX_K"):
        OL.knn_mean_distance(x, 33, "cuda:0")
