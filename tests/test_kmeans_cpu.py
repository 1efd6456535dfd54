"""CPU: the numpy restatement of the k-means labelling (tests/kmeans_ref.py) against the fixture pinned by running the reference's
RecMap.cluster and sklearn (tests/golden/kmeans_pinned.npz, tests/tools/gen_kmeans_pinned.py), and the host side of
pram_amd.localization.labelling that needs no GPU.

The label rule.  The restatement's distances are ((x0 - c0)^2 + (x1 - c1)^2) + (x2 - c2)^2, sklearn's are |c|^2 - 2 x.c; both round
within about 10 ulp of R^2, R the largest centred norm.  A label may therefore differ from the fixture only where the restatement's
margin between the best and the second-best distance is at most 2^-40 R^2 (a factor of 512 above that rounding), and for at most
0.1 % of the points.  On the fixture's scenes the smallest margin is 9e-7 R^2: nothing is excused."""
from pathlib import Path

import numpy as np
import pytest

from tests import kmeans_ref as KR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_kmeans_workspace_bytes", "pram_kmeans_init_pp", "pram_kmeans_lloyd", "pram_kmeans_assign")
check_labels, scene_inputs = KR.check_labels, KR.scene_inputs


@pytest.fixture(scope="module")
def restated():
    """the restatement on every scene and init of the fixture, computed once"""
    out = {}
    for tag in KR.SCENES:
        xyz, ids, mode, k = scene_inputs(tag)
        out[tag] = KR.cluster_points(xyz, k, mode=mode)
    for tag, (n, k, seed, n_far) in KR.GIVEN.items():
        xyz, init = KR.given_init(n, k, seed, n_far)
        out[tag] = KR.cluster_points(xyz, k, init=init)
    return out


def test_symbols_declared_and_exported(hip_lib):
    # the entries' declarations, types and exports and header == ops for the PRAM_KMEANS_* constants: tests/test_abi_contract_cpu.py
    from pram_amd import _lib, ops
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    assert KR.BLOCK == ops.KMEANS_BLOCK and ops.KMEANS_MAX_K >= 4096 and ops.KMEANS_MAX_TRIALS >= 2 + int(np.log(ops.KMEANS_MAX_K))
    assert (ROOT / "pram_amd" / "csrc" / "kmeans.hip").exists()
    L = hip_lib
    assert L.pram_kmeans_workspace_bytes(5000, 16) > 8 * 5000 + 8 * 5000
    for n, k in ((0, 1), (5, 0), (5, 6), (2 ** 31, 4), (10000, ops.KMEANS_MAX_K + 1)):
        assert L.pram_kmeans_workspace_bytes(n, k) == 0, (n, k)


@pytest.mark.parametrize("tag", list(KR.SCENES))
def test_restatement_reproduces_the_reference(golden, restated, tag):
    g, r = golden("kmeans_pinned"), restated[tag]
    xyz, ids, mode, k = scene_inputs(tag)
    assert np.array_equal(g[tag + "_id"], ids)
    assert int(g[tag + "_n_iter"]) == r["n_iter"]
    assert np.abs(r["centers"] - g[tag + "_centers"]).max() <= 1e-10
    assert check_labels(xyz, mode, r, g[tag + "_label"]) == 0      # measured: the reference stays inside the cap with nothing excused
    assert np.unique(r["labels"]).size == k and r["relocations"] == 0


@pytest.mark.parametrize("tag", list(KR.GIVEN))
def test_restatement_reproduces_sklearn_on_inits_that_empty_clusters(golden, restated, tag):
    g, r = golden("kmeans_pinned"), restated[tag]
    n, k, seed, n_far = KR.GIVEN[tag]
    xyz, init = KR.given_init(n, k, seed, n_far)
    assert int(g[tag + "_n_iter"]) == r["n_iter"] and r["relocations"] == n_far
    assert np.abs(r["centers"] - g[tag + "_centers"]).max() <= 1e-10
    check_labels(xyz, "xyz", r, g[tag + "_label"])


def test_restatement_pieces():
    # a blocked sum is not numpy's pairwise sum, and depends on the block
    v = np.random.RandomState(3).uniform(0.0, 1.0, size=3 * KR.BLOCK + 17)
    within, run = KR.block_prefix(v)
    acc = 0.0
    for b in range(4):
        s = 0.0
        for t in v[b * KR.BLOCK:(b + 1) * KR.BLOCK]:
            s = s + t
        acc = acc + s
    assert KR.blocked_sum(v) == acc == run[-1]
    # ties go to the lowest centre, and the mode zeroes what it does not name
    c = np.array([[1.0, 0, 0], [-1.0, 0, 0], [1.0, 0, 0]])
    assert KR.assign(np.zeros((2, 3)), c)[0].tolist() == [0, 0]
    assert KR.apply_mode(np.ones((2, 3)), "xz").tolist() == [[1, 0, 1]] * 2
    # all points identical: the second seed is point 0, cluster 1 is empty and takes point 0
    r = KR.cluster_points(np.full((5, 3), 2.5), 2)
    assert r["seeds"][1] == 0 and r["relocations"] >= 1 and r["inertia"] == 0.0


def test_landmarks_from_labels_equals_load_segmentation(golden):
    from pram_amd.localization.labelling import landmarks_from_labels
    g = golden("kmeans_pinned")
    for tag in KR.SCENES:
        landmarks, sids = landmarks_from_labels(g[tag + "_id"], g[tag + "_label"])
        keys, off, flat = g[tag + "_seg_keys"].tolist(), g[tag + "_seg_off"], g[tag + "_seg_ids"]
        assert list(landmarks) == keys      # the order in which the labels first appear
        for i, s in enumerate(keys):
            assert landmarks[s] == flat[off[i]:off[i + 1]].tolist(), (tag, s)
        assert list(sids.items()) == list(zip(g[tag + "_id"].tolist(), g[tag + "_label"].tolist()))
        want_seg, want_p3d = KR.segmentation_dicts(g[tag + "_id"].tolist(), g[tag + "_label"].tolist())
        assert landmarks == want_seg and sids == want_p3d
    with pytest.raises(ValueError):
        landmarks_from_labels([1, 2], [0])


def test_label_points_order_filter_and_refusals(monkeypatch):
    """The host side of label_points with the device call replaced: the reference's order over the tracks, its min_obs filter, the
    unmasked xyz, and what it refuses before any device is touched."""
    from pram_amd.localization import labelling as LB
    n, k, seed, mode = KR.SCENES["obs16"]
    xyz = KR.scene(n, k, seed, mode)
    ids, track_len = KR.track_scene(n, seed)
    tracks = {int(p): (np.zeros(int(t), dtype=np.int64), np.zeros(int(t), dtype=np.int64)) for p, t in zip(ids, track_len)}
    xyzs = {int(p): xyz[i] for i, p in enumerate(ids)}
    seen = {}

    def fake(x, kk, device, mode="xyz", **kw):
        seen.update(x=x, k=kk, mode=mode, kw=kw)
        return {"labels": np.arange(x.shape[0], dtype=np.int32) % kk}

    monkeypatch.setattr(LB, "cluster_points", fake)
    out = LB.label_points(tracks, xyzs, k, "cuda:0", mode="xz", min_obs=KR.MIN_OBS, seed=5)
    keep = track_len >= KR.MIN_OBS
    assert 0 < keep.sum() < n
    assert np.array_equal(out["id"], ids[keep]) and np.array_equal(out["xyz"], xyz[keep]) and np.array_equal(seen["x"], xyz[keep])
    assert seen["mode"] == "xz" and seen["kw"] == {"seed": 5} and set(out) == {"id", "label", "xyz"}
    with pytest.raises(ValueError, match="one at a time"):
        LB.label_points(tracks, xyzs, k, "cuda:0", method="birch", threshold=0.01)
    with pytest.raises(ValueError, match="does not exist"):
        LB.label_points(tracks, xyzs, k, "cuda:0", method="dbscan")
    del xyzs[int(ids[keep][0])]
    with pytest.raises(ValueError, match="no xyz"):
        LB.label_points(tracks, xyzs, k, "cuda:0")


def test_host_preparation_matches_the_restatement():
    from pram_amd.localization import labelling as LB
    for n, k, seed in ((1, 1, 0), (50, 7, 3), (4000, 16, 0), (5000, 513, 9)):
        first, rand = LB.pp_randoms(n, k, seed)
        f2, r2 = KR.pp_randoms(n, k, seed)
        assert first == f2 and np.array_equal(rand, r2) and rand.shape == (k - 1, 2 + int(np.log(k)))
    x = KR.scene(100, 4, 1)
    assert np.array_equal(LB.apply_mode(x, "y"), KR.apply_mode(x, "y")) and (LB.apply_mode(x, "y")[:, [0, 2]] == 0).all()
    with pytest.raises(Exception):
        LB.cluster_points(x, 4, "cpu")
