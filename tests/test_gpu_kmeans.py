"""GPU: k-means labelling on the device (pram_amd.localization.labelling, csrc/kmeans.hip) against the numpy restatement
tests/kmeans_ref.py, exactly (labels, the centres' bits, iteration count, inertia, relocations, the seeds), and against the fixture
pinned by the reference (tests/golden/kmeans_pinned.npz) under the label rule of tests/test_kmeans_cpu.py; the assignment step and
the seeding on their own, degenerate inputs, the stopping rules, and the C entries' refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kmeans_ref as KR

pytestmark = pytest.mark.gpu
check_labels, scene_inputs = KR.check_labels, KR.scene_inputs


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(got, want, what=""):
    """the device's result equals the restatement's, bit for bit"""
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], want["labels"]), what
    assert np.array_equal(bits(got["centers"]), bits(want["centers"])), what
    assert got["n_iter"] == want["n_iter"] and got["relocations"] == want["relocations"], (what, got["n_iter"], want["n_iter"])
    assert bits(got["inertia"]) == bits(want["inertia"]), (what, got["inertia"], want["inertia"])
    if want["seeds"] is not None:
        assert np.array_equal(got["seeds"], want["seeds"]), what


# Every n with every k <= n, then k = n; the three modes in turn.  n: around the 64 lanes of a wave, the 256 points of a workgroup's
# pass and the 1024 of a block, and several blocks; k: around the 512 centres of an LDS chunk, and beyond the 1024 points of a block.
NS, KS, MODES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000), (1, 2, 3, 16, 64, 65, 512, 513), ("xyz", "xz", "y")
SHAPES = [(n, k) for n in NS for k in KS if k <= n] + [(n, n) for n in NS if n not in KS and n <= 4096]
SHAPES = [(n, k, MODES[i % 3]) for i, (n, k) in enumerate(SHAPES)]


@pytest.mark.parametrize("n,k,mode", SHAPES)
def test_shapes_equal_the_restatement(dev, n, k, mode):
    from pram_amd.localization.labelling import cluster_points
    xyz = KR.scene(n, max(1, min(k, 24)), 100 + n + k, mode)
    want = KR.cluster_points(xyz, k, mode=mode, seed=n % 7)
    got = cluster_points(xyz, k, dev, mode=mode, seed=n % 7)
    same(got, want, (n, k, mode))
    assert got["centers"].shape == (k, 3) and got["labels"].shape == (n,)
    for d, c in enumerate("xyz"):
        if c not in mode:
            assert (got["centers"][:, d] == 0).all()


@pytest.fixture(scope="module")
def restated():
    out = {}
    for tag in KR.SCENES:
        xyz, ids, mode, k = scene_inputs(tag)
        out[tag] = KR.cluster_points(xyz, k, mode=mode)
    for tag, (n, k, seed, n_far) in KR.GIVEN.items():
        xyz, init = KR.given_init(n, k, seed, n_far)
        out[tag] = KR.cluster_points(xyz, k, init=init)
    return out


@pytest.mark.parametrize("tag", list(KR.SCENES))
def test_fixture_scenes_through_label_points(dev, golden, restated, tag):
    from pram_amd.localization.labelling import label_points, landmarks_from_labels
    g = golden("kmeans_pinned")
    n, k, seed, mode = KR.SCENES[tag]
    xyz = KR.scene(n, k, seed, mode)
    if tag == "obs16":
        ids, track_len = KR.track_scene(n, seed)
    else:
        ids, track_len = np.arange(1, n + 1, dtype=np.int64), np.full(n, KR.MIN_OBS)
    tracks = {int(p): (np.zeros(int(t), dtype=np.int64), np.zeros(int(t), dtype=np.int64)) for p, t in zip(ids, track_len)}
    out = label_points(tracks, {int(p): xyz[i] for i, p in enumerate(ids)}, k, dev, mode=mode, min_obs=KR.MIN_OBS)
    kept_xyz, kept_ids, _, _ = scene_inputs(tag)
    assert np.array_equal(out["id"], g[tag + "_id"]) and np.array_equal(out["id"], kept_ids) and np.array_equal(out["xyz"], kept_xyz)
    assert np.array_equal(out["label"], restated[tag]["labels"])
    check_labels(kept_xyz, mode, {"labels": out["label"], "centers": restated[tag]["centers"]}, g[tag + "_label"])
    landmarks, sids = landmarks_from_labels(out["id"], out["label"])
    assert sorted(landmarks) == list(range(k)) and sum(len(v) for v in landmarks.values()) == len(sids) == kept_ids.size


@pytest.mark.parametrize("tag", list(KR.GIVEN))
def test_given_inits_that_empty_clusters(dev, golden, restated, tag):
    from pram_amd.localization.labelling import cluster_points
    g = golden("kmeans_pinned")
    n, k, seed, n_far = KR.GIVEN[tag]
    xyz, init = KR.given_init(n, k, seed, n_far)
    got = cluster_points(xyz, k, dev, init=init)
    same(got, restated[tag], tag)
    assert got["relocations"] == n_far and got["seeds"] is None
    assert got["n_iter"] == int(g[tag + "_n_iter"]) and np.abs(got["centers"] - g[tag + "_centers"]).max() <= 1e-10
    check_labels(xyz, "xyz", got, g[tag + "_label"])


def test_init_pp_alone(dev):
    """the seeds as point indices, and the centres as the seeds' coordinates"""
    from pram_amd import ops
    for n, k, seed in ((2049, 65, 4), (1500, 9, 1), (3, 3, 2)):
        xc, _, _ = KR.prepare(KR.scene(n, 12, 300 + n), "xyz", 1e-4)
        first, rand = KR.pp_randoms(n, k, seed)
        seeds, centers = ops.kmeans_init_pp(torch.from_numpy(xc).to(dev), k, first, torch.from_numpy(rand).to(dev))
        want = KR.init_pp(xc, k, first, rand)
        assert seeds.dtype == torch.int32 and np.array_equal(seeds.cpu().numpy(), want), (n, k)
        assert np.array_equal(bits(centers.cpu().numpy()), bits(xc[want]))
    # a target beyond the total potential is clipped to the last point: rand = 2 puts every candidate there
    xc = KR.prepare(KR.scene(1030, 3, 7), "xyz", 1e-4)[0]
    rand = np.full((1, 2), 2.0)
    seeds, _ = ops.kmeans_init_pp(torch.from_numpy(xc).to(dev), 2, 5, torch.from_numpy(rand).to(dev))
    assert seeds.cpu().tolist() == [5, 1029] == KR.init_pp(xc, 2, 5, rand).tolist()


def test_assign_nearest_ties_go_to_the_lowest_index(dev):
    from pram_amd.localization.labelling import assign_nearest
    # an integer lattice: every distance is exact, a point in the middle of a cell is as far from all of its corners
    g = np.arange(0, 12, 2, dtype=np.float64)
    corners = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)                    # 216 centres
    centers = np.concatenate([corners[::-1], corners, corners[::-1], corners])[:700]                    # every one several times, past an LDS chunk
    mids = corners[(corners < 10).all(axis=1)] + 1.0
    pts = np.concatenate([mids, corners, mids + [1.0, 0, 0]] * 2)      # 932 points: more than centres
    labels, dist = assign_nearest(pts, centers, dev)
    want_l, want_d = KR.assign(pts, centers)
    assert labels.dtype == torch.int32 and dist.dtype == torch.float64 and labels.is_cuda
    assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(bits(dist.cpu().numpy()), bits(want_d))
    d = ((pts[:, None, :] - centers[None, :, :]) ** 2).sum(-1)
    first_min = np.array([np.flatnonzero(row == row.min())[0] for row in d])
    assert np.array_equal(want_l, first_min) and ((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).all() and (dist.cpu().numpy()[:mids.shape[0]] == 3.0).all()
    # fewer points than centres, and tensors on the device as inputs
    l2, d2 = assign_nearest(torch.from_numpy(pts[:5]).to(dev), torch.from_numpy(centers).to(dev), dev)
    assert np.array_equal(l2.cpu().numpy(), want_l[:5]) and np.array_equal(bits(d2.cpu().numpy()), bits(want_d[:5]))


def test_degenerate_inputs(dev):
    """What the restatement defines: identical points (the second seed is point 0, cluster 1 is empty at every step and takes the
    point farthest away, which is point 0), and more clusters than distinct points."""
    from pram_amd.localization.labelling import cluster_points
    for n, k in ((1500, 1), (1500, 2), (7, 2)):
        xyz = np.full((n, 3), [3.25, -1.5, 7.0])
        want = KR.cluster_points(xyz, k)
        got = cluster_points(xyz, k, dev)
        same(got, want, (n, k))
        assert got["inertia"] == 0.0 and (got["labels"] == 0).all() and got["relocations"] == (0 if k == 1 else got["n_iter"])
    rs = np.random.RandomState(5)
    distinct = rs.uniform(-20.0, 20.0, size=(10, 3))
    xyz = distinct[rs.randint(0, 10, size=1200)]
    want = KR.cluster_points(xyz, 16, seed=3)
    got = cluster_points(xyz, 16, dev, seed=3)
    same(got, want, "duplicates")
    assert got["relocations"] >= 6 and np.unique(got["labels"]).size <= 10


def test_stopping_rules(dev):
    from pram_amd.localization.labelling import cluster_points
    xyz = KR.scene(3000, 12, 77)
    xc, mean, _ = KR.prepare(xyz, "xyz", 1e-4)
    full = KR.cluster_points(xyz, 12)
    assert full["n_iter"] > 3
    # max_iter = 1: one update, then one more assignment against the moved centres
    want = KR.cluster_points(xyz, 12, max_iter=1)
    got = cluster_points(xyz, 12, dev, max_iter=1)
    same(got, want, "max_iter=1")
    assert got["n_iter"] == 1 and np.array_equal(got["labels"], KR.assign(xc, got["centers"] - mean)[0])
    assert not np.array_equal(got["labels"], KR.assign(xc, xc[want["seeds"]])[0])      # not the first step's labels
    # a tolerance that the first shift already meets
    want = KR.cluster_points(xyz, 12, tol=1e6)
    got = cluster_points(xyz, 12, dev, tol=1e6)
    same(got, want, "tol")
    assert got["n_iter"] == 1 and np.array_equal(got["labels"], KR.assign(xc, got["centers"] - mean)[0])
    # max_iter in the middle of a group of iterations, and tol = 0 (strict convergence only)
    for kw in ({"max_iter": 3}, {"tol": 0.0}):
        same(cluster_points(xyz, 12, dev, **kw), KR.cluster_points(xyz, 12, **kw), kw)


def test_two_runs_and_every_group_size_give_equal_bits(dev):
    from pram_amd.localization.labelling import cluster_points
    xyz = KR.scene(4100, 20, 55)
    want = KR.cluster_points(xyz, 20)
    assert want["n_iter"] > 8
    timings = {}
    runs = [cluster_points(xyz, 20, dev), cluster_points(xyz, 20, dev), cluster_points(xyz, 20, dev, iter_group=1),
            cluster_points(xyz, 20, dev, iter_group=5, timings=timings), cluster_points(xyz, 20, dev, iter_group=300)]
    for r in runs:
        same(r, want)
    assert timings["group_reads"] == -(-want["n_iter"] // 5) and set(timings) >= {"init", "lloyd", "readback"}


def test_labels_feed_build_store_inputs(dev):
    from tests import mapbuild_ref as MR
    from pram_amd.localization import mapbuild as MB
    from pram_amd.localization.candidates import ReferenceStore
    from pram_amd.localization.labelling import label_points, landmarks_from_labels
    s = MR.scene()
    out = label_points(s["tracks"], s["xyz"], 6, dev, mode="xz", min_obs=3)
    assert out["id"].size >= 6 and all(len(s["tracks"][int(p)][1]) >= 3 for p in out["id"])
    landmarks, sids = landmarks_from_labels(out["id"], out["label"])
    assert sorted(landmarks) == list(range(6))
    built = MB.build_store_inputs(s["frames"], s["tracks"], landmarks, s["xyz"], dev, s["ignored"], **MR.VRF_PARAMS)
    assert list(built["seg_ref_frame_ids"]) == list(landmarks) and any(len(v) for v in built["seg_ref_frame_ids"].values())
    # a store wants a landmark for every point of its table: label them all
    out = label_points(s["tracks"], s["xyz"], 6, dev, mode="xz", min_obs=1)
    landmarks, sids = landmarks_from_labels(out["id"], out["label"])
    built = MB.build_store_inputs(s["frames"], s["tracks"], landmarks, s["xyz"], dev, s["ignored"], **MR.VRF_PARAMS)
    store = ReferenceStore(s["frames"], point3D_sids=sids, **{k: built[k] for k in MB.STORE_KEYS})
    assert np.array_equal(store.pt_ids, s["point_ids"]) and set(store.pt_sid.tolist()) == set(range(6))


def test_c_entries_refuse_without_launching(dev, hip_lib):
    """Every refusal of the entries: PRAM_E_ARG, a message, and the outputs untouched."""
    from pram_amd import ops
    L = hip_lib
    n, k, T = 3000, 8, 4
    x = torch.from_numpy(KR.prepare(KR.scene(n, k, 1), "xyz", 1e-4)[0]).to(dev)
    rand = torch.rand(k - 1, T, device=dev, dtype=torch.float64)
    need = L.pram_kmeans_workspace_bytes(n, k)
    ws = torch.empty(need + 8, device=dev, dtype=torch.uint8)
    seeds = torch.full((k,), -77, device=dev, dtype=torch.int32)
    centers = torch.full((k, 3), 7.0, device=dev, dtype=torch.float64)
    labels = torch.full((n,), -77, device=dev, dtype=torch.int32)
    dist = torch.full((n,), 7.0, device=dev, dtype=torch.float64)
    state = torch.full((ops.KMEANS_STATE_WORDS,), -77, device=dev, dtype=torch.int32)
    inertia = torch.full((2,), 7.0, device=dev, dtype=torch.float64)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()

    def init(x_=P(x), n_=n, k_=k, first=0, rand_=P(rand), T_=T, ws_=P(ws), bytes_=need, seeds_=P(seeds), centers_=P(centers)):
        return L.pram_kmeans_init_pp(x_, n_, k_, first, rand_, T_, ws_, bytes_, seeds_, centers_, st)

    def lloyd(x_=P(x), n_=n, k_=k, centers_=P(centers), tol=1e-3, max_iter=10, first=0, iters=2, ws_=P(ws), bytes_=need, labels_=P(labels), dist_=P(dist),
              state_=P(state), inertia_=P(inertia)):
        return L.pram_kmeans_lloyd(x_, n_, k_, centers_, tol, max_iter, first, iters, 1, ws_, bytes_, labels_, dist_, state_, inertia_, st)

    def assign(x_=P(x), n_=n, centers_=P(centers), k_=k, labels_=P(labels), dist_=P(dist)):
        return L.pram_kmeans_assign(x_, n_, centers_, k_, labels_, dist_, st)

    shapes = ({"n_": 0}, {"n_": -3}, {"k_": 0}, {"k_": n + 1, "n_": n}, {"n_": 5, "k_": 6}, {"n_": 2 ** 31}, {"n_": 2 ** 31 + 5000}, {"k_": ops.KMEANS_MAX_K + 1, "n_": 10 ** 6})
    for fn in (init, lloyd, assign):
        for kw in shapes:
            assert fn(**kw) == -1 and b"needs 1 <= n < 2^31" in L.pram_last_error(), (fn.__name__, kw)
    for fn, names in ((init, ("x_", "ws_", "seeds_", "centers_", "rand_")), (lloyd, ("x_", "centers_", "ws_", "labels_", "dist_", "state_", "inertia_")),
                      (assign, ("x_", "centers_", "labels_", "dist_"))):
        for nm in names:
            assert fn(**{nm: None}) == -1 and b"null" in L.pram_last_error(), (fn.__name__, nm)
    for fn, names in ((init, ("x_", "ws_", "centers_", "rand_")), (lloyd, ("x_", "centers_", "ws_", "dist_", "inertia_")), (assign, ("x_", "centers_", "dist_"))):
        for nm in names:
            ptr = {"x_": P(x), "ws_": P(ws), "centers_": P(centers), "rand_": P(rand), "dist_": P(dist), "inertia_": P(inertia)}[nm] + 4
            assert fn(**{nm: ptr}) == -1 and b"8-byte" in L.pram_last_error(), (fn.__name__, nm)
    for fn, names in ((init, ("seeds_",)), (lloyd, ("labels_", "state_")), (assign, ("labels_",))):
        for nm in names:
            ptr = {"seeds_": P(seeds), "labels_": P(labels), "state_": P(state)}[nm] + 2
            assert fn(**{nm: ptr}) == -1 and b"misaligned" in L.pram_last_error(), (fn.__name__, nm)
    for fn in (init, lloyd):
        assert fn(bytes_=need - 1) == -1 and b"workspace" in L.pram_last_error()
    assert init(first=-1) == -1 and init(first=n) == -1 and b"first seed" in L.pram_last_error()
    assert init(T_=0) == -1 and init(T_=ops.KMEANS_MAX_TRIALS + 1) == -1 and b"n_trials" in L.pram_last_error()
    assert lloyd(max_iter=0) == -1 and lloyd(first=-1) == -1 and lloyd(iters=-1) == -1 and lloyd(first=9, iters=2) == -1 and b"max_iter" in L.pram_last_error()
    assert lloyd(tol=-1.0) == -1 and lloyd(tol=float("nan")) == -1 and b"tol_abs" in L.pram_last_error()
    torch.cuda.synchronize()
    assert (seeds == -77).all() and (centers == 7.0).all() and (labels == -77).all() and (dist == 7.0).all() and (state == -77).all() and (inertia == 7.0).all()
    # and the Python layer before any call
    from pram_amd.localization.labelling import cluster_points
    for bad in ({"k": 0}, {"k": 3001}, {"k": 4, "max_iter": 0}, {"k": 4, "tol": -1.0}, {"k": 4, "init": "random"}, {"k": 4, "init": np.zeros((3, 3))}):
        with pytest.raises(ValueError):
            cluster_points(x.cpu().numpy(), device=dev, **bad)
    with pytest.raises(ValueError):
        cluster_points(np.full((10, 3), np.nan), 2, dev)
