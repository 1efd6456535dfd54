"""Labelling a map's points on the device: the landmarks every later step of the offline chain starts from.

Reference: recognition/recmap.py.
  * RecMap.cluster(method='kmeans') (recmap.py:85-122): sklearn's KMeans(n_clusters=k, random_state=0) on the coordinates of the
    points with at least min_obs observations, the coordinates ``mode`` does not name zeroed -> :func:`cluster_points`,
    :func:`label_points`.
  * RecMap.load_segmentation (recmap.py:63-74): the label file as the two dicts the rest of the chain takes
    -> :func:`landmarks_from_labels`.
:func:`assign_nearest` is one assignment step in public: labels for new points, and the last step of Birch when a caller brings
sub-cluster centroids from elsewhere.  The kernels are csrc/kmeans.hip; torch here is plumbing.  The host does the O(n)
preparation in numpy (the mask of ``mode``, sklearn's centring, the tolerance, every random number: none depends on the data) and
reads one state word per group of ITER_GROUP iterations.

Where this differs from sklearn, on purpose: the arithmetic has one fixed order (include/pram_hip.h, restated in
tests/kmeans_ref.py), so a result is the same bits on every run and on every machine; it depends on PRAM_KMEANS_BLOCK.  sklearn's
distances are |c|^2 - 2 x.c from BLAS, its sums follow its thread chunks, and it multiplies by the reciprocal of a count where
this divides.  On well separated data the labels are the same (tests/golden/kmeans_pinned.npz: every label of the reference on
three scenes); a point within rounding of the boundary between two centres can differ.  sklearn takes its tolerance from the
variance before centring, this from the centred points: the same number up to rounding.

Not here: method='birch' (its CF-tree is built by inserting samples one at a time and its global step is an agglomerative merge:
neither is data-parallel).  Open3D's statistical outlier removal (recmap.py:43-61), which the reference runs before this step on its
outdoor datasets, is localization/outliers.py: its filter_points takes and returns the two dicts label_points takes."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from pram_amd import ops

ITER_GROUP = 8      # Lloyd iterations enqueued between two looks at the done word


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        from pram_amd._lib import PramHipError
        raise PramHipError("labelling: expected a CUDA device (pram_amd has no CPU path)")
    return device


def _points(xyz, name: str = "xyz") -> np.ndarray:
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f"{name}: expected [n, 3], got {x.shape}")
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: more than 2^31 - 1 points")
    if not np.isfinite(x).all():
        raise ValueError(f"{name}: coordinates must be finite")
    return x


def apply_mode(xyz: np.ndarray, mode: str) -> np.ndarray:
    """A copy with the coordinates ``mode`` does not name zeroed (recmap.py:102-107)."""
    x = np.array(xyz, dtype=np.float64, copy=True)
    for d, c in enumerate("xyz"):
        if mode.find(c) < 0:
            x[:, d] = 0
    return x


def pp_randoms(n: int, k: int, seed: int):
    """Every random number sklearn's k-means++ draws from RandomState(seed): the first centre, then 2 + int(ln k) uniform numbers
    for each of the k - 1 steps -> (first, rand float64 [k - 1, T])."""
    rs = np.random.RandomState(seed)
    trials = 2 + int(np.log(k))
    first = int(rs.choice(n, p=np.full(n, 1.0) / float(n)))
    rand = np.array([rs.uniform(size=trials) for _ in range(k - 1)], dtype=np.float64).reshape(k - 1, trials)
    return first, rand


@torch.no_grad()
def cluster_points(xyz, k: int, device, mode: str = "xyz", seed: int = 0, init="k-means++", max_iter: int = 300, tol: float = 1e-4,
                   iter_group: int = ITER_GROUP, timings: Optional[dict] = None) -> dict:
    """xyz float64 [n, 3] -> dict(labels int32 [n], centers float64 [k, 3] in the caller's coordinates, n_iter, inertia,
    relocations: how many times an empty cluster took a point), all on the host.  ``init``: 'k-means++' (seeded by ``seed``) or
    float64 [k, 3] centres in the caller's coordinates, as in sklearn.  The result does not depend on ``iter_group``.  ``seeds``
    (k-means++ only): the seeds as point indices.  ``timings``: a dict that receives the seconds spent in the host's preparation, seeding,
    iterations and read-backs (each stage is then waited for, which a run without it does not do)."""
    import time
    device = _device(device)
    t_begin = time.perf_counter()
    x = apply_mode(_points(xyz), mode)
    n, k, max_iter, iter_group = x.shape[0], int(k), int(max_iter), int(iter_group)
    if k < 1 or k > n or k > ops.KMEANS_MAX_K:
        raise ValueError(f"cluster_points: needs 1 <= k <= min(n, {ops.KMEANS_MAX_K}), got n = {n}, k = {k}")
    if max_iter < 1 or iter_group < 1 or not tol >= 0:
        raise ValueError("cluster_points: needs max_iter >= 1, iter_group >= 1 and tol >= 0")
    mean = x.mean(axis=0)
    xc = x - mean
    tol_abs = float(np.mean(np.var(xc, axis=0)) * tol)

    def clock():
        if timings is not None:
            torch.cuda.synchronize(device)
        return time.perf_counter()

    with torch.cuda.device(device):
        t0 = clock()
        xd = torch.from_numpy(np.ascontiguousarray(xc)).to(device)
        ws = ops.kmeans_workspace(n, k, device)
        seeds = None
        if isinstance(init, str):
            if init != "k-means++":
                raise ValueError(f"cluster_points: init is 'k-means++' or an array, got {init!r}")
            first, rand = pp_randoms(n, k, int(seed))
            rand_d = torch.from_numpy(rand if rand.size else np.zeros((1, rand.shape[1]))).to(device)
            seeds, centers = ops.kmeans_init_pp(xd, k, first, rand_d, ws)
        else:
            c0 = _points(init, "init")
            if c0.shape[0] != k:
                raise ValueError(f"init: expected [{k}, 3], got {c0.shape}")
            centers = torch.from_numpy(np.ascontiguousarray(c0 - mean)).to(device)
        t1 = clock()
        buf = ops.kmeans_buffers(n, device)
        it, reads, t_read = 0, 0, 0.0
        while True:
            g = min(iter_group, max_iter - it)
            ops.kmeans_lloyd(xd, centers, tol_abs, max_iter, it, g, False, buf, ws)
            it += g
            r0 = clock()
            done = int(buf["state"][ops.KMEANS_DONE].item())      # the one read-back of the group
            t_read += time.perf_counter() - r0
            reads += 1
            if done or it >= max_iter:
                break
        ops.kmeans_lloyd(xd, centers, tol_abs, max_iter, it, 0, True, buf, ws)
        t2 = clock()
        state = buf["state"].cpu().numpy()
        out = {"labels": buf["labels"].cpu().numpy(), "centers": centers.cpu().numpy() + mean, "n_iter": int(state[ops.KMEANS_ITER]),
               "inertia": float(buf["inertia"][0].item()), "relocations": int(state[ops.KMEANS_RELOC]),
               "seeds": None if seeds is None else seeds.cpu().numpy()}
        t3 = clock()
    if timings is not None:
        timings.update(prepare=t0 - t_begin, init=t1 - t0, lloyd=t2 - t1 - t_read, readback=t_read + (t3 - t2), group_reads=reads, iter_group=iter_group)
    return out


def label_points(tracks: Dict[int, tuple], point3D_xyzs: dict, k: int, device, mode: str = "xyz", min_obs: int = 3, method: str = "kmeans",
                 **kw) -> dict:
    """tracks: point id -> (image_ids, point2D_idxs) and point3D_xyzs: point id -> xyz, as mapbuild.build_store_inputs takes them
    -> {'id', 'label', 'xyz'}: the reference's label file.  The points whose track has at least ``min_obs`` entries, in the
    iteration order of ``tracks`` (the reference's order over points3D.values()); 'xyz' is not masked, as in the reference.
    kw: seed, init, max_iter, tol of :func:`cluster_points`."""
    if method == "birch":
        raise ValueError("label_points: method='birch' is not built: Birch's CF-tree is built by inserting samples one at a time and its "
                         "global step is an agglomerative merge, neither of which is data-parallel; run sklearn's Birch on the host and "
                         "give its sub-cluster centroids to assign_nearest for the last step")
    if method != "kmeans":
        raise ValueError(f"label_points: method {method!r} does not exist (the reference has 'kmeans' and 'birch')")
    ids = [pid for pid, trk in tracks.items() if len(trk[1]) >= min_obs]
    missing = [pid for pid in ids if pid not in point3D_xyzs]
    if missing:
        raise ValueError(f"point3D_xyzs: {len(missing)} points of the tracks have no xyz, e.g. point id {missing[0]}")
    xyz = np.array([np.asarray(point3D_xyzs[pid], dtype=np.float64).reshape(3) for pid in ids], dtype=np.float64).reshape(-1, 3)
    r = cluster_points(xyz, k, device, mode=mode, **kw)
    return {"id": np.array(ids), "label": r["labels"], "xyz": xyz}


def landmarks_from_labels(ids, labels):
    """The label file's 'id' and 'label' -> (landmarks, point3D_sids): RecMap.load_segmentation's seg_p3d (landmark id -> point ids
    in file order, what build_store_inputs and select_reference_frames take) and p3d_seg (point id -> landmark id, what
    ReferenceStore(point3D_sids=) takes).  A repeated point id keeps its last label and its first place, as a dict does."""
    ids, labels = np.asarray(ids).reshape(-1), np.asarray(labels).reshape(-1)
    if ids.shape != labels.shape:
        raise ValueError(f"landmarks_from_labels: {ids.shape[0]} ids, {labels.shape[0]} labels")
    point3D_sids = {int(p): int(s) for p, s in zip(ids.tolist(), labels.tolist())}
    landmarks: Dict[int, list] = {}
    for p, s in point3D_sids.items():
        landmarks.setdefault(s, []).append(p)
    return landmarks, point3D_sids


@torch.no_grad()
def assign_nearest(xyz, centers, device):
    """xyz [n, 3] and centers [k, 3] (numpy arrays or tensors, float64) -> (labels int32 [n], squared distance float64 [n]) on the
    device; the lowest centre index wins a tie.  No centring and no mask: both in the caller's coordinates."""
    device = _device(device)

    def dev(a, name):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float64:
            raise ValueError(f"{name}: expected float64 [n, 3], got {t.dtype} {tuple(t.shape)}")
        return t.to(device).contiguous()

    x, c = dev(xyz, "xyz"), dev(centers, "centers")
    n, k = int(x.shape[0]), int(c.shape[0])
    if n < 1 or k < 1:
        raise ValueError("assign_nearest: needs at least one point and one centre")
    with torch.cuda.device(device):
        if k > n:      # the entry takes k <= n: fewer points than centres are padded with copies of the last one
            x = torch.cat([x, x[-1:].expand(k - n, 3)]).contiguous()
        labels, dist = ops.kmeans_assign(x, c)
    return labels[:n], dist[:n]
