"""Batched absolute pose on the device: P3P RANSAC, refinement and the choice among a query's candidates.

Reference: SingleMap3D.localize_with_ref_frame's call of pycolmap.absolute_pose_estimation (localization/singlemap3d.py:168-193)
and the candidate loop's verify_and_update with its early exit (localization/multimap3d.py:183-239, 294-313).  The reference
solves pair after pair on the host; here the five kernels of csrc/pose.hip take the padded outputs of pram_cand_correspond for
all B * seg_k pairs at once, and ONE read-back at the end brings the per-pair results and the selection to the host.

This is not COLMAP's estimator: a fixed trial budget replaces its adaptive stop, and two refine / re-score passes at the end
replace its in-loop local optimisation (DESIGN.md 4.12 states the deviations)."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import candidates as _cand

_N_PARAMS = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8}
DEFAULT_REFINE_ITERS = 20


def camera_table(cameras: Sequence) -> tuple:
    """cameras: one (model_name, width, height, params) tuple per query, as localization/utils.py parses the query lists.
    -> (model ids int32 [B], params float64 [B, 8] zero padded), numpy; an unknown model or a short parameter list -> ValueError."""
    ids = np.zeros(len(cameras), dtype=np.int32)
    params = np.zeros((len(cameras), ops.POSE_CAM_PARAMS), dtype=np.float64)
    for i, cam in enumerate(cameras):
        name, prm = str(cam[0]), np.asarray(cam[3], dtype=np.float64).reshape(-1)
        if name not in ops.CAMERA_MODELS:
            raise ValueError(f"camera {i}: model {name!r} is not supported (supported: {', '.join(ops.CAMERA_MODELS)})")
        k = _N_PARAMS[name]
        if prm.size < k:
            raise ValueError(f"camera {i}: {name} needs {k} parameters, got {prm.size}")
        ids[i] = ops.CAMERA_MODELS[name]
        params[i, :k] = prm[:k]
    return ids, params


def camera_form(cameras) -> str:
    """Which of the three forms a ``cameras`` argument has: 'resident' (device_cameras' result: two device tensors and the host
    ids), 'table' (camera_table's result: two numpy arrays) or 'tuples' (anything else: a sequence of camera tuples, which
    camera_table checks)."""
    if isinstance(cameras, tuple) and len(cameras) == 3 and torch.is_tensor(cameras[0]):
        return "resident"
    if isinstance(cameras, tuple) and len(cameras) == 2 and isinstance(cameras[0], np.ndarray):
        return "table"
    return "tuples"


def device_cameras(cameras, device) -> tuple:
    """camera tuples (or camera_table's result) -> (model ids int32 [B], params float64 [B, 8]) on the device plus the ids as a
    host list: what estimate_poses takes as ``cameras`` when the upload (a blocking copy from pageable memory) is to happen once,
    outside the per-batch path."""
    ids, params = cameras if camera_form(cameras) == "table" else camera_table(cameras)
    return torch.from_numpy(ids).to(device), torch.from_numpy(params).to(device), [int(i) for i in ids]


def _device_cameras(cameras, device):
    return cameras if camera_form(cameras) == "resident" else device_cameras(cameras, device)


class ReadBack:
    """Per-row results on the host after ONE device-to-host copy: est's qvec [P, 4] and tvec [P, 3], the named int32 columns
    ``ints`` (name -> [P]; they travel as float64, which holds every int32 exactly), optionally an int ``tail`` [P, k] of which
    row i holds ints[tail_count][i] valid entries, and optionally ``block``, a second int table of any shape packed behind the
    rows (the selection per query behind the results per pair).  rb[i] -> dict(qvec, tvec, every named int, and 'tail' cut to
    its count); rb.block -> int64, block's shape."""

    def __init__(self, est: dict, ints: Dict[str, torch.Tensor], tail=None, tail_count=None, block=None):
        self.names, self.tail_count = tuple(ints), tail_count
        cols = [est["qvec"], est["tvec"], torch.stack([ints[k] for k in self.names], 1).double()]
        packed = torch.cat(cols if tail is None else cols + [tail.double()], 1)
        self.tail_at = packed.shape[1] - (0 if tail is None else tail.shape[1])
        if block is None:
            self.rows, self.block = packed.cpu().numpy(), None
        else:
            flat = torch.cat([packed.reshape(-1), block.double().reshape(-1)]).cpu().numpy()
            self.rows, self.block = flat[:packed.numel()].reshape(packed.shape), flat[packed.numel():].reshape(block.shape).astype(np.int64)

    def __len__(self) -> int:
        return len(self.rows)

    def __getitem__(self, i: int) -> dict:
        row = self.rows[i]
        r = {"qvec": row[:4].copy(), "tvec": row[4:7].copy()}
        r.update({k: int(v) for k, v in zip(self.names, row[7:self.tail_at])})
        if self.tail_count is not None:
            r["tail"] = row[self.tail_at:self.tail_at + r[self.tail_count]].astype(np.int64)
        return r


@torch.no_grad()
def estimate_poses(matched_keypoints: torch.Tensor, matched_xyzs: torch.Tensor, counts: torch.Tensor, cameras, *, seg_k: int,
                   threshold: float, trials: int = 1000, min_inlier_ratio: float = 0.01, refine_iters: int = DEFAULT_REFINE_ITERS,
                   seed: int = 0) -> Dict[str, torch.Tensor]:
    """matched_keypoints float32 [P, t0, 2] (pixels, without the + 0.5), matched_xyzs float64 [P, t0, 3], counts int32 [P] (valid rows
    per pair), P = B * seg_k; cameras: B tuples, camera_table's result, or device_cameras' result (already resident).  threshold: the
    RANSAC inlier bound in pixels.
    -> dict of device tensors: qvec [P, 4] (w, x, y, z), tvec [P, 3], inliers uint8 [P, t0], num_inliers, success int32 [P], plus
    best (the winning hypothesis slot, trial * 4 + root; -1 none).  Nothing is read back.  With device_cameras' result there is no
    host synchronisation inside; with camera tuples the table is uploaded here, a blocking copy."""
    P, t0 = ops._pose_chk(matched_keypoints, matched_xyzs, counts)
    cam_model, cam_params, host_ids = _device_cameras(cameras, matched_keypoints.device)
    pts = ops.pose_prepare(matched_keypoints, counts, cam_model, cam_params, host_ids, seg_k)
    poses, n_sol = ops.pose_hypotheses(pts, matched_xyzs, counts, trials, seed)
    h_inl, h_res, best = ops.pose_score(pts, matched_xyzs, counts, poses, n_sol, cam_model, cam_params, seg_k, threshold)
    out = ops.pose_refine(matched_keypoints, pts, matched_xyzs, counts, poses, h_inl, best, cam_model, cam_params, seg_k, threshold,
                          min_inlier_ratio, refine_iters)
    out["best"] = best
    return out


@torch.no_grad()
def localize_candidates(features: dict, recognition, store, matcher, cameras, *, seg_k: int, min_kpts: int, threshold: float,
                        min_inliers: int, semantic_matching: bool = True, overlap_ratio: float = 0.5, trials: int = 1000,
                        min_inlier_ratio: float = 0.01, refine_iters: int = DEFAULT_REFINE_ITERS, seed: int = 0) -> List[dict]:
    """match_candidates' stages, then the pose of every (query, candidate) pair on the padded correspondences, then the reference's
    choice among a query's candidates.  Two host synchronisations in all: the plan read-back of the matching stage and ONE
    read-back of the per-pair results and the selection.

    -> per query a dict: success (a candidate was kept), tracking_status (True / False / None), qvec (w, x, y, z), tvec, num_inliers,
    inliers (bool [n_matches]), order, reference_frame_id, sid and the matched_* tensors of the kept candidate cut to n_matches,
    plus candidates: the per-candidate list of match_candidates, each with success, qvec, tvec, num_inliers and inliers (padded)."""
    return _localize(features, recognition, store, matcher, cameras, seg_k=seg_k, min_kpts=min_kpts, threshold=threshold,
                     min_inliers=min_inliers, semantic_matching=semantic_matching, overlap_ratio=overlap_ratio, trials=trials,
                     min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed)[0]


@torch.no_grad()
def _localize(features: dict, recognition, store, matcher, cameras, *, seg_k: int, min_kpts: int, threshold: float, min_inliers: int,
              semantic_matching: bool, overlap_ratio: float, trials: int, min_inlier_ratio: float, refine_iters: int, seed: int):
    """localize_candidates' body -> (its result, state): state keeps what stays on the device for a later stage (the refinement):
    chosen int32 [B, 3], plan, tokens, cor (pram_cand_correspond's outputs), est (the per-pair estimates), seg_k, plus the
    read-back selection sel [B, 3] on the host."""
    planned = _cand.plan_candidates(features, recognition, store, seg_k=seg_k, min_kpts=min_kpts, semantic_matching=semantic_matching,
                                    overlap_ratio=overlap_ratio)
    cor, host, m = _cand._match_planned(features, planned, store, matcher)
    B = features["counts"].numel()
    est = estimate_poses(cor["matched_keypoints"], cor["matched_xyzs"], cor["count"], cameras, seg_k=seg_k, threshold=threshold, trials=trials,
                         min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed)
    chosen = ops.pose_select(est["success"], est["num_inliers"], seg_k, min_inliers)
    # the one read-back: 7 doubles and 3 ints per pair, 3 ints per query
    rb = ReadBack(est, {"success": est["success"], "num_inliers": est["num_inliers"], "count": cor["count"]}, block=chosen)
    sel = rb.block
    lists = _cand._candidate_lists(cor, host, m, store, B, seg_k)
    out = []
    for b in range(B):
        for w, c in enumerate(lists[b]):
            p = b * seg_k + w
            v = rb[p]
            c.update(success=bool(v["success"]), qvec=v["qvec"], tvec=v["tvec"], num_inliers=v["num_inliers"],
                     inliers=est["inliers"][p, :c["n_query_kpts"]], n_matches_host=v["count"])
        kept, status = int(sel[b, 0]), int(sel[b, 1])
        r = {"success": kept >= 0, "tracking_status": None if status < 0 else bool(status), "candidates": lists[b]}
        if kept >= 0:
            c = lists[b][kept]
            n = c["n_matches_host"]
            r.update(qvec=c["qvec"], tvec=c["tvec"], num_inliers=c["num_inliers"], inliers=c["inliers"][:n].bool(), order=c["order"],
                     reference_frame_id=c["reference_frame_id"], sid=c["sid"])
            r.update({k: v[:n] for k, v in c.items() if k.startswith("matched_")})
        else:
            r.update(qvec=None, tvec=None, num_inliers=0, inliers=None, order=-1, reference_frame_id=None, sid=None)
        out.append(r)
    state = {"chosen": chosen, "plan": planned["plan"], "tokens": planned["vote"]["tokens"], "cor": cor, "est": est, "seg_k": seg_k, "sel": sel}
    return out, state
