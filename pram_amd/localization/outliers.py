"""Statistical outlier removal of a map's points on the device: the first step of the offline chain.

Reference: recognition/recmap.py.
  * RecMap.compute_statics_inlier (recmap.py:609-614): Open3D's remove_statistical_outlier on an array of points
    -> :func:`statistical_inliers`.
  * RecMap.remove_statics_outlier (recmap.py:43-61): the same on the model's points, in the order of points3D.keys(); the
    outliers leave the model and the ids of the others stay -> :func:`remove_statistical_outliers` on the dict
    triangulation.triangulate_map returns, :func:`filter_points` on the pair of dicts labelling.label_points takes.
process_dataset turns it on for every outdoor dataset with nb_neighbors=20, std_ratio=2.0 (recmap.py:1036-1037): the defaults here.

The algorithm is Open3D's PointCloud::RemoveStatisticalOutliers as include/pram_hip.h states it, written from knowledge of its
source: Open3D is not installed and was never run beside this, so nothing here is pinned to it.  The numpy
restatement tests/outliers_ref.py is what the device equals bit for bit, and that is cross-checked on the CPU against a k-d tree.
  * every point's mean distance to its min(nb_neighbors, n) nearest points, itself included; a point whose mean is 0 (it has
    that many exact duplicates) is not valid; over the valid points the mean and the sample deviation of those means; the inliers
    are the valid points below mean + std_ratio * std, strictly.  With fewer than two valid points nothing is an inlier.
  * the search is all-pairs and exact (csrc/knn.hip), where Open3D asks a k-d tree; nb_neighbors is at most ops.KNN_MAX_K = 32,
    the list a thread keeps in registers.  Neighbour indices are not returned.
torch here is plumbing: one upload, two entries, one read-back at the end."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization.labelling import _points

STAT_KEYS = ("mean", "std", "threshold", "n_valid")


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        from pram_amd._lib import PramHipError
        raise PramHipError("outliers: expected a CUDA device (pram_amd has no CPU path)")
    return device


def _params(nb_neighbors, std_ratio):
    k, ratio = int(nb_neighbors), float(std_ratio)
    if k < 1 or not ratio > 0:
        raise ValueError(f"outliers: needs nb_neighbors >= 1 and std_ratio > 0, got {nb_neighbors} and {std_ratio}")      # Open3D's
    if k > ops.KNN_MAX_K:
        raise ValueError(f"outliers: nb_neighbors = {k} is above PRAM_KNN_MAX_K = {ops.KNN_MAX_K}, the neighbours a thread keeps in registers")
    return k, ratio


def _cloud(xyz, device: torch.device) -> torch.Tensor:
    """A numpy array or a float64 tensor [n, 3] -> the points on the device, checked as labelling._points checks them."""
    if torch.is_tensor(xyz):
        if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float64:
            raise ValueError(f"xyz: expected float64 [n, 3], got {xyz.dtype} {tuple(xyz.shape)}")
        if xyz.shape[0] >= 2 ** 31:
            raise ValueError("xyz: more than 2^31 - 1 points")
        x = xyz.to(device).contiguous()
        if not bool(torch.isfinite(x).all()):
            raise ValueError("xyz: coordinates must be finite")
    else:
        x = torch.from_numpy(np.ascontiguousarray(_points(xyz))).to(device)
    if x.shape[0] < 1:
        raise ValueError("xyz: needs at least one point")
    return x


@torch.no_grad()
def knn_mean_distance(xyz, nb_neighbors: int, device) -> torch.Tensor:
    """xyz [n, 3] (a numpy array or a float64 device tensor) -> float64 [n] on the device: every point's mean distance to its
    min(nb_neighbors, n) nearest points, itself included at distance 0."""
    device = _device(device)
    k, _ = _params(nb_neighbors, 1.0)
    with torch.cuda.device(device):
        return ops.knn_mean_distance(_cloud(xyz, device), k)


@torch.no_grad()
def statistical_inliers(xyz, device, nb_neighbors: int = 20, std_ratio: float = 2.0, timings: Optional[dict] = None) -> dict:
    """xyz [n, 3] -> on the host: ``inlier_ids`` int64 (ascending: what Open3D returns), ``mask`` bool [n], ``avg_distance``
    float64 [n], ``mean``, ``std``, ``threshold`` (NaN without two valid points) and ``n_valid``.  ``timings``: a dict that
    receives the seconds of the upload, the k-NN kernel, the selection and the read-back (each stage is then waited for, which a
    run without it does not do)."""
    import time
    device = _device(device)
    k, ratio = _params(nb_neighbors, std_ratio)

    def clock():
        if timings is not None:
            torch.cuda.synchronize(device)
        return time.perf_counter()

    with torch.cuda.device(device):
        t0 = clock()
        x = _cloud(xyz, device)
        t1 = clock()
        avg = ops.knn_mean_distance(x, k)
        t2 = clock()
        sel = ops.sor_select(avg, ratio)
        t3 = clock()
        # ---- the one read-back
        count = sel["count"].cpu().numpy()
        stats = sel["stats"].cpu().numpy()
        out = {"inlier_ids": sel["inlier_idx"][:int(count[0])].cpu().numpy().astype(np.int64), "mask": sel["mask"].cpu().numpy().astype(bool),
               "avg_distance": avg.cpu().numpy(), "mean": float(stats[ops.SOR_MEAN]), "std": float(stats[ops.SOR_STD]),
               "threshold": float(stats[ops.SOR_THRESHOLD]), "n_valid": int(count[1])}
        t4 = clock()
    if timings is not None:
        timings.update(upload=t1 - t0, knn=t2 - t1, select=t3 - t2, readback=t4 - t3)
    return out


def _info(r: dict, ids: np.ndarray) -> dict:
    return {"removed_ids": ids[~r["mask"]], "avg_distance": r["avg_distance"], **{k: r[k] for k in STAT_KEYS}}


def filter_points(tracks: Dict[int, tuple], point3D_xyzs: dict, device, nb_neighbors: int = 20, std_ratio: float = 2.0):
    """tracks: point id -> (image_ids, point2D_idxs) and point3D_xyzs: point id -> xyz, as labelling.label_points takes them
    -> (tracks, point3D_xyzs, info) without the outliers.  The cloud is every point of ``point3D_xyzs`` in its iteration order
    (the reference's order over points3D.keys()); the ids and the order of the others stay.  info: ``removed_ids``,
    ``avg_distance`` (in the cloud's order), ``mean``, ``std``, ``threshold``, ``n_valid``.  The inputs are not modified."""
    ids = list(point3D_xyzs)
    xyz = np.array([np.asarray(point3D_xyzs[p], dtype=np.float64).reshape(3) for p in ids], dtype=np.float64).reshape(-1, 3)
    r = statistical_inliers(xyz, device, nb_neighbors=nb_neighbors, std_ratio=std_ratio)
    info = _info(r, np.array(ids))
    gone = set(info["removed_ids"].tolist())
    return ({p: t for p, t in tracks.items() if p not in gone}, {p: v for p, v in point3D_xyzs.items() if p not in gone}, info)


def remove_statistical_outliers(model: dict, device, nb_neighbors: int = 20, std_ratio: float = 2.0) -> dict:
    """model: the dict triangulation.triangulate_map returns -> the same dict restricted to the inliers of ``point3D_xyzs`` (in
    ``point_ids`` order): ``point_ids`` (kept, not renumbered), ``point3D_xyzs``, ``track_error``; ``tracks`` and
    ``point3D_frame_ids`` without the removed ids; in ``frames`` a keypoint whose point was removed gets ``point3D_ids`` -1 and
    ``xyzs`` 0.  Every other key passes through.  Added: ``removed_ids``, ``avg_distance`` (over the input's points), ``mean``,
    ``std``, ``threshold``, ``n_valid``.  The input is not modified; the result goes into labelling.label_points and
    mapbuild.build_store_inputs as triangulate_map's does."""
    ids = np.asarray(model["point_ids"])
    r = statistical_inliers(model["point3D_xyzs"], device, nb_neighbors=nb_neighbors, std_ratio=std_ratio)
    keep = r["mask"]
    if keep.shape != ids.shape:
        raise ValueError(f"model: {ids.shape[0]} point_ids, {keep.shape[0]} point3D_xyzs")
    info = _info(r, ids)
    out = restrict_model(model, keep)
    out.update(info)
    return out


def restrict_model(model: dict, keep: np.ndarray) -> dict:
    """model: triangulate_map's dict; keep: bool over ``point_ids`` -> the dict restricted to the kept points, as
    :func:`remove_statistical_outliers` documents it (bundle.bundle_adjust cleans its result the same way).  The input is not
    modified."""
    ids = np.asarray(model["point_ids"])
    removed = ids[~keep]
    gone = set(removed.tolist())
    out = dict(model)
    out["point_ids"], out["point3D_xyzs"] = ids[keep], np.asarray(model["point3D_xyzs"])[keep]
    if "track_error" in model:
        out["track_error"] = np.asarray(model["track_error"])[keep]
    for key in ("tracks", "point3D_frame_ids"):
        if key in model:
            out[key] = {p: t for p, t in model[key].items() if p not in gone}
    if "frames" in model:
        frames = []
        for f in model["frames"]:
            pid = np.asarray(f["point3D_ids"])
            lost = np.isin(pid, removed)
            frames.append({**f, "point3D_ids": np.where(lost, -1, pid), "xyzs": np.where(lost[:, None], 0.0, np.asarray(f["xyzs"]))})
        out["frames"] = frames
    return out
