"""Numpy restatement of the reference's offline localizer, for the tests of pram_amd.localization.retrieval.

Written from localization/pose_estimator.py: get_covisibility_frames (:18-42), feature_matching (:45-86), find_2D_3D_matches
(:89-134), pose_estimator_hloc (:138-270), pose_refinement (:273-376), pose_estimator_iterative (:380-612).  Plain host loops over
plain numpy; a ``map`` is refine_ref's (frames with ids, optionally point3D_frame_ids and ``poses``: frame id -> (qvec, tvec)); a
``query`` is cand_ref's.  The matcher is a callable (data dict, tag) -> matches0 over the frame's VALID rows (int64 [m]); the
solver a callable (keypoints, xyzs, tag) -> dict(success, inliers, num_inliers, qvec, tvec); tag = ('slot', j) for a retrieved
frame, ('covis', j) for a frame of the covisibility stage, ('stack',) / ('refine',) for the solver's calls on stacks.

The deviations of DESIGN.md 4.23 are restated, not the reference's accidents: equal covisibility counts go (count descending,
position of the frame in map['frames'] ascending); the iterative form solves every slot and then selects; a query that takes the
best slot uses that slot's pose and inliers; a failed query takes the first retrieved frame's stored pose (num_inliers -1 for the
iterative form, 0 for hloc), an empty list gives qvec None and num_inliers 0; the keypoints are kept without the + 0.5."""
from __future__ import annotations

from collections import defaultdict

import numpy as np

from tests import refine_ref as RR

STACK_KEYS = RR.STACK_KEYS
HLOC_OBS_TH = 3


def _position(map_: dict) -> dict:
    return {fid: i for i, fid in enumerate(RR.frame_ids(map_))}


def valid_rows(frame: dict, pf: dict) -> np.ndarray:
    """feature_matching's ``masks = db_3D_ids != -1`` (:63-64); an id without an entry in points3D (the reference raises KeyError
    at :122) is no usable point either."""
    return np.array([i for i, p in enumerate(np.asarray(frame["point3D_ids"]).tolist()) if p != -1 and p in pf], dtype=np.int64)


def get_covisibility_frames(map_: dict, frame_id, covisibility_frame: int, include_self: bool = False, with_counts: bool = False, pf: dict = None) -> list:
    position = _position(map_)
    pf = RR.point_frames(map_) if pf is None else pf
    covis = defaultdict(int)
    for pid in np.asarray(map_["frames"][position[frame_id]]["point3D_ids"]).tolist():
        if pid == -1 or pid not in pf:
            continue
        for g in pf[pid]:
            if include_self or g != frame_id:
                covis[g] += 1
    top = sorted(covis, key=lambda g: (-covis[g], position[g]))[:covisibility_frame]
    return [(g, covis[g]) for g in top] if with_counts else top


def covisibility_pairs(map_: dict, k: int) -> list:
    pf = RR.point_frames(map_)
    return [(fid, g) for fid in RR.frame_ids(map_) for g in get_covisibility_frames(map_, fid, k, pf=pf)]


def feature_matching(query: dict, frame: dict, pf: dict, matcher, tag) -> tuple:
    """-> (matches0 over the frame's valid rows, matches over the frame's rows)."""
    valid = valid_rows(frame, pf)
    n = query["keypoints"].shape[0]
    if len(valid) == 0 or n == 0:
        return np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    rk = np.asarray(frame["keypoints"], dtype=np.float32)
    data = {"descriptors0": query["descriptors"], "keypoints0": query["keypoints"], "scores0": query["scores"],
            "image_shape0": (1, 3, query["width"], query["height"]),
            "descriptors1": np.asarray(frame["descriptors"], dtype=np.float32)[valid], "keypoints1": rk[valid, :2], "scores1": rk[valid, 2],
            "image_shape1": (1, 3, frame["width"], frame["height"])}
    m0 = np.asarray(matcher(data, tag)).astype(np.int64)
    return m0, np.where(m0 >= 0, valid[np.clip(m0, 0, len(valid) - 1)], -1)


def find_2D_3D_matches(query: dict, frame: dict, pf: dict, matcher, obs_th: int, tag) -> dict:
    m0, matches = feature_matching(query, frame, pf, matcher, tag)
    pids = np.asarray(frame["point3D_ids"])
    keep = [i for i in range(len(matches)) if matches[i] != -1 and pids[matches[i]] != -1 and len(pf.get(int(pids[matches[i]]), ())) >= obs_th]
    q = np.array(keep, dtype=np.int64)
    rows = matches[q]
    rk = np.asarray(frame["keypoints"], dtype=np.float32)
    return {"matches0": m0, "matched_keypoints": query["keypoints"][q], "matched_keypoint_ids": q,
            "matched_xyzs": np.asarray(frame["xyzs"], dtype=np.float64)[rows], "matched_point3D_ids": pids[rows].astype(np.int64),
            "matched_sids": np.asarray(frame.get("keypoint_segs", np.zeros(len(pids), np.int32)))[rows].astype(np.int32), "matched_ref_keypoints": rk[rows, :2]}


def stack(parts: list) -> dict:
    """np.vstack of the slots that have rows (:183-186, :210-211), plus matched_src, the slot of origin."""
    live = [(j, p) for j, p in enumerate(parts) if p["matched_keypoints"].shape[0] > 0]
    out = {k: (np.concatenate([np.asarray(p[k]) for _, p in live]) if live else np.zeros(*RR._EMPTY[k])) for k in STACK_KEYS}
    out["matched_src"] = np.concatenate([np.full(p["matched_keypoints"].shape[0], j, dtype=np.int32) for j, p in live]) if live else np.zeros(0, np.int32)
    return out


def _stored_pose(map_: dict, db_ids: list):
    poses = map_.get("poses")
    if not db_ids or poses is None:
        return None, None
    return np.asarray(poses[db_ids[0]][0], dtype=np.float64), np.asarray(poses[db_ids[0]][1], dtype=np.float64)


def _inlier_lists(lst: dict, ret: dict) -> dict:
    inl = np.asarray(ret["inliers"], dtype=bool)
    return {"keypoints_query": lst["matched_keypoints"][inl], "points3D_ids": lst["matched_point3D_ids"][inl]}


def pose_estimator_hloc(query: dict, map_: dict, db_ids: list, matcher, solver) -> dict:
    pf, position = RR.point_frames(map_), _position(map_)
    per_slot = [find_2D_3D_matches(query, map_["frames"][position[g]], pf, matcher, HLOC_OBS_TH, ("slot", j)) for j, g in enumerate(db_ids)]
    out = stack(per_slot)
    out.update(per_slot=per_slot, order=-1, reference_frame_id=db_ids[0] if db_ids else None)
    ret = solver(out["matched_keypoints"], out["matched_xyzs"], ("stack",)) if db_ids and len(out["matched_keypoint_ids"]) else {"success": False}
    if ret["success"]:
        out.update(success=True, status=1, qvec=ret["qvec"], tvec=ret["tvec"], num_inliers=ret["num_inliers"], inliers=np.asarray(ret["inliers"], dtype=bool),
                   **_inlier_lists(out, ret))
    else:
        q, t = _stored_pose(map_, db_ids)
        out.update(success=False, status=0, qvec=q, tvec=t, num_inliers=0, inliers=None, keypoints_query=np.zeros((0, 2), np.float32),
                   points3D_ids=np.zeros(0, np.int64))
    return out


def pose_refinement(query: dict, map_: dict, frame_id, matcher, solver, *, covisibility_frame: int, obs_th: int, qvec, tvec) -> dict:
    pf, position = RR.point_frames(map_), _position(map_)
    db_ids = get_covisibility_frames(map_, frame_id, covisibility_frame, pf=pf)
    per_slot = [find_2D_3D_matches(query, map_["frames"][position[g]], pf, matcher, obs_th, ("covis", j)) for j, g in enumerate(db_ids)]
    out = stack(per_slot)
    out.update(per_slot=per_slot, covisible_frame_ids=db_ids)
    ret = solver(out["matched_keypoints"], out["matched_xyzs"], ("refine",))
    if ret["success"]:
        out.update(success=True, qvec=ret["qvec"], tvec=ret["tvec"], num_inliers=ret["num_inliers"], inliers=np.asarray(ret["inliers"], dtype=bool),
                   **_inlier_lists(out, ret))
    else:      # :351-363
        n = len(out["matched_keypoint_ids"])
        out.update(success=False, qvec=qvec, tvec=tvec, num_inliers=0, inliers=np.zeros(n, dtype=bool), keypoints_query=np.zeros((0, 2), np.float32),
                   points3D_ids=np.zeros(0, np.int64))
    return out


def select(success, num_inliers, count, inlier_th: int, min_best_inliers: int = 10) -> tuple:
    """The walk of :429-556 and :558 over one query's slots -> (kept slot or -1, status, best slot or -1)."""
    best, best_inl = -1, 0
    for j in range(len(count)):
        if count[j] < 8 or not success[j]:
            continue
        if num_inliers[j] > best_inl:
            best, best_inl = j, int(num_inliers[j])
        if num_inliers[j] >= inlier_th:
            return j, 1, best
    if best >= 0 and best_inl >= min_best_inliers:
        return best, 2, best
    return -1, 0, best


def pose_estimator_iterative(query: dict, map_: dict, db_ids: list, matcher, solver, *, inlier_th: int = 50, min_best_inliers: int = 10,
                             do_covisibility_opt: bool = False, covisibility_frame: int = 50, obs_th: int = 0) -> dict:
    pf, position = RR.point_frames(map_), _position(map_)
    per_slot = [find_2D_3D_matches(query, map_["frames"][position[g]], pf, matcher, obs_th, ("slot", j)) for j, g in enumerate(db_ids)]
    rets = [solver(p["matched_keypoints"], p["matched_xyzs"], ("slot", j)) for j, p in enumerate(per_slot)]
    kept, status, best = select([r["success"] for r in rets], [r.get("num_inliers", 0) for r in rets], [len(p["matched_keypoint_ids"]) for p in per_slot],
                                inlier_th, min_best_inliers)
    out = {"per_slot": per_slot, "slot_results": rets, "kept": kept, "status": status, "best": best, "success": kept >= 0}
    if kept < 0:
        q, t = _stored_pose(map_, db_ids)
        out.update(qvec=q, tvec=t, num_inliers=-1 if db_ids else 0, order=best + 1 if best >= 0 else -1, inliers=None,
                   reference_frame_id=db_ids[max(best, 0)] if db_ids else None, keypoints_query=np.zeros((0, 2), np.float32), points3D_ids=np.zeros(0, np.int64))
        if do_covisibility_opt:
            out["refinement"] = None
        return out
    ret, lst = rets[kept], per_slot[kept]
    out.update({k: lst[k] for k in STACK_KEYS})
    out.update(qvec=ret["qvec"], tvec=ret["tvec"], num_inliers=ret["num_inliers"], order=kept + 1, reference_frame_id=db_ids[kept],
               inliers=np.asarray(ret["inliers"], dtype=bool), **_inlier_lists(lst, ret))
    if do_covisibility_opt:
        x = pose_refinement(query, map_, db_ids[kept], matcher, solver, covisibility_frame=covisibility_frame, obs_th=obs_th, qvec=ret["qvec"], tvec=ret["tvec"])
        out.update(refinement=x, qvec=x["qvec"], tvec=x["tvec"], num_inliers=x["num_inliers"], keypoints_query=x["keypoints_query"], points3D_ids=x["points3D_ids"])
    return out


# the retrieval lists the tests use on refine_ref.covisible_scene: query 3 sees 8 points in frame 107 only, query 4 is empty
SCENE_RETRIEVAL = ([101, 100, 102, 106], [105, 104, 103], [107], [107, 106], [])
