"""Pose refinement over covisible frames, on the device: by matching (refine_by_matching) and by projection
(refine_by_projection, at the end of this file with its own notes).

Reference: SingleMap3D.refine_pose_by_matching (localization/singlemap3d.py:268-365) as MultiMap3D.run calls it after a query is
located (multimap3d.py:245-271), with build_covisibility_graph (singlemap3d.py:228-258) and find_reference_frames
(singlemap3d.py:500-511).  The first pose of a query rests on ONE reference frame; here ALL keypoints of every located query are
matched against the WHOLE of each frame covisible with that reference frame, in ONE grouped matcher call for all (query, frame)
pairs of the batch, the matches are stacked per query (the localisation's own matches last, when the reference keeps them), one
pose is estimated per stack and the stack's points vote for the new reference frames.

Stages: pram_refine_plan, pram_cand_gather, the matcher, pram_cand_correspond, pram_refine_merge, the four pose kernels,
pram_refine_frame_vote.  Two host synchronisations: the read-back of the plan table (40 bytes per pair), which fixes the padded
size of the grouped call, and ONE read-back of the per-query results.

Deviations: the pose stage is pram_amd's (a fixed ``trials`` budget instead of min_num_trials / max_num_trials /
confidence; DESIGN.md 4.12's deviations carry over); where the reference leaves the order of equal counts to argsort /
argpartition the order is (count descending, store frame index ascending); a refinement whose solver fails or that found no
match in any frame — the reference then raises IndexError (singlemap3d.py:307) or KeyError (multimap3d.py:259) — comes back with
success False and zeros, its frame vote run over all matched ids as the reference's code would, and with an empty vote
reference_frame_id stays the localisation's; the kept matches' xyz are the reference frame's rows (the reference re-reads the
points' xyz, the same numbers in a consistent map).  One map per store; no QueryPipeline stage."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import candidates as _cand
from pram_amd.localization import pose as _pose

_MATCHED = ops.MATCH_RESULT_KEYS + (ops.MATCH_SRC,)


def enable_mask(enable, B: int, dtype=np.int32):
    """A per-query ``enable`` argument (None, a list, a numpy array of any dtype, a tensor on any device) -> numpy [B] of dtype;
    None stays None.  Anything but one entry per query is a ValueError."""
    if enable is None:
        return None
    on = np.asarray(enable.cpu() if torch.is_tensor(enable) else enable).astype(dtype).reshape(-1)
    if on.size != B:
        raise ValueError("enable: expected one entry per query")
    return on


def _preamble(features: dict, store, covisibility_frame: Optional[int]):
    """What both refinements check first -> (counts, device, B, n_cov); the caller returns [] for B == 0."""
    counts = features["counts"]
    ops._chk(counts, "counts", torch.int32)
    n_cov = int(store.covisibility_frame if covisibility_frame is None else covisibility_frame)
    if n_cov < 1:
        raise ValueError("covisibility_frame < 1")
    return counts, counts.device, counts.numel(), n_cov


def _device_enable(enable, B: int, dev):
    on = enable_mask(enable, B)
    return None if on is None else torch.from_numpy(on).to(dev)


def _solve_and_vote(lists: dict, keys, cameras, store, tables: dict, n_cov: int, ref_frame: torch.Tensor, extra: Dict[str, torch.Tensor],
                    own, pose_kw: dict) -> List[Optional[dict]]:
    """The tail both refinements share, from a query's stacked matches to its result: ONE pose per query on ``lists``
    (matched_keypoints, matched_xyzs, matched_point3D_ids, count; seg_k = 1, so the sampler's pair index is the query index), the
    frame vote of the stack's points, ONE read-back (7 doubles, the ints below, the voted frames), and per query None (ref_frame
    < 0: not located, or not enabled) or the result dict with lists[keys] cut to the count — reference_frame_id is the vote's
    first frame and, with an empty vote, stays the localisation's — to which own(b, v) adds the calling form's own entries from
    the read-back row v (``extra`` by name)."""
    est = _pose.estimate_poses(lists["matched_keypoints"], lists["matched_xyzs"], lists["count"], cameras, seg_k=1, **pose_kw)
    k = max(1, min(n_cov, store.n_frames))
    best_f, _, n_best = ops.refine_frame_vote(lists["matched_point3D_ids"], lists["count"], est["inliers"], est["success"], tables, k)
    rb = _pose.ReadBack(est, dict(success=est["success"], num_inliers=est["num_inliers"], count=lists["count"], ref_frame=ref_frame, **extra, n_best=n_best),
                        tail=best_f, tail_count="n_best")
    out = []
    for b in range(len(rb)):
        v = rb[b]
        if v["ref_frame"] < 0:
            out.append(None)
            continue
        frames = [store.frame_ids[int(i)] for i in v["tail"]]
        r = {"success": bool(v["success"]), "qvec": v["qvec"], "tvec": v["tvec"], "num_inliers": v["num_inliers"],
             "inliers": est["inliers"][b, :v["count"]].bool(), "refinement_reference_frame_ids": frames,
             "reference_frame_id": frames[0] if frames else store.frame_ids[v["ref_frame"]]}
        r.update({key: lists[key][b, :v["count"]] for key in keys})
        r.update(own(b, v))
        out.append(r)
    return out


@torch.no_grad()
def refine_by_matching(features: dict, state: dict, store, matcher, cameras, *, threshold: float, covisibility_frame: Optional[int] = None,
                       trials: int = 1000, min_inlier_ratio: float = 0.01, refine_iters: int = _pose.DEFAULT_REFINE_ITERS, seed: int = 0,
                       enable=None) -> List[Optional[dict]]:
    """features, store, matcher, cameras: as localize_candidates takes them; state: the device-side result of that localisation
    (pose._localize: chosen, plan, tokens, cor, est, seg_k).  covisibility_frame: frames matched per query and length of the
    returned frame list (None: the store's).  enable: per query, refine it or not (None: every located query).  threshold: the
    RANSAC inlier bound in pixels; the sampler's pair index is the query index.

    -> per query None (not located, or not enabled) or the reference's ``ret``: success, qvec (w, x, y, z), tvec, num_inliers,
    inliers (bool [m]); matched_keypoints [m, 2], matched_keypoint_ids, matched_xyzs, matched_point3D_ids, matched_sids,
    matched_ref_keypoints, matched_src (slot of origin; n_covisible_slots = the localisation's matches): device tensors cut to
    the m merged rows; refinement_reference_frame_ids (frame ids, at most covisibility_frame), reference_frame_id; n_covisible
    (frames matched), used_init (the localisation's matches were appended), and slots: per covisible frame its frame id,
    n_ref_kpts, matches0 / matching_scores0 [n_query_kpts] and n_matches (0-d device tensor)."""
    counts, dev, B, n_cov = _preamble(features, store, covisibility_frame)
    if B == 0:
        return []
    tables = store.tables(dev)
    chosen = state["chosen"]
    plan, ref_frame, used, init_on = ops.refine_plan(chosen, state["plan"], counts.contiguous(), tables, n_cov, _device_enable(enable, B, dev))
    cor, host, m = _cand._match_planned(features, {"plan": plan, "vote": {"tokens": state["tokens"]}}, store, matcher)
    merged = ops.refine_merge(cor, state["cor"], chosen, init_on, n_cov)
    f = ops.CAND_PLAN_FIELDS
    col = lambda name: host[f.index(name)]

    def own(b, v):
        slots = []
        for p in range(b * n_cov, b * n_cov + v["n_covisible"]):
            l0 = int(col("lens0")[p])
            slots.append({"reference_frame_id": store.frame_ids[int(col("frame")[p])], "n_query_kpts": l0, "n_ref_kpts": int(col("lens1")[p]),
                          "matches0": m["matches0"][p, :l0], "matching_scores0": m["matching_scores0"][p, :l0], "n_matches": cor["count"][p]})
        return {"n_covisible": v["n_covisible"], "used_init": bool(v["used_init"]), "slots": slots}

    return _solve_and_vote(merged, _MATCHED, cameras, store, tables, n_cov, ref_frame, {"n_covisible": used, "used_init": init_on}, own,
                           dict(threshold=threshold, trials=trials, min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed))


def image_size_table(cameras) -> np.ndarray:
    """camera tuples (model_name, width, height, params) -> int32 [B, 2] (width, height)."""
    return np.array([[int(c[1]), int(c[2])] for c in cameras], dtype=np.int32).reshape(-1, 2)


_PROJ_MATCHED = tuple(k for k in ops.MATCH_RESULT_KEYS if k != ops.MATCH_REF_KPTS)


@torch.no_grad()
def refine_by_projection(features: dict, state: dict, store, cameras, *, threshold: float, covisibility_frame: Optional[int] = None,
                         trials: int = 1000, min_inlier_ratio: float = 0.01, refine_iters: int = _pose.DEFAULT_REFINE_ITERS, seed: int = 0,
                         enable=None, image_sizes=None) -> List[Optional[dict]]:
    """SingleMap3D.refine_pose_by_projection (singlemap3d.py:367-498) for all located queries of a batch: the points the frames
    covisible with the localisation's reference frame observe (and that frame's own) are projected with the localisation's pose,
    every keypoint is matched against the points projecting within 2 * threshold pixels of it (descriptor distance, 0.995 ratio
    test), one pose is estimated on those matches and they vote for the new reference frames.

    Stages: pram_projref_mark, pram_projref_project, pram_projref_match, pram_projref_correspond, the four pose kernels,
    pram_refine_frame_vote.  ONE host synchronisation, the read-back of the per-query results; every buffer is sized on the host
    (candidates per query: min(n_points, (n_cov + 1) * store.max_frame_rows)).  No network runs, PRAM_PRECISION does not apply:
    the projection is float64, the descriptor products fp32.

    Arguments as refine_by_matching's, without the matcher.  image_sizes: int32 [B, 2] (width, height), needed when ``cameras`` is
    device_cameras' result (camera tuples carry them).  -> per query None (not located, or not enabled) or success, qvec, tvec,
    num_inliers, inliers, the matched_* lists (keypoints, keypoint ids, xyzs, point ids, landmarks: what the reference returns),
    refinement_reference_frame_ids, reference_frame_id, plus n_union (points marked), n_projected (points in the frustum) and dists
    [n_query_kpts, 2] (smallest and second smallest in-range descriptor distance, +inf where there is none).

    Deviations: the pose stage's, as in refine_by_matching; rows with point id -1 or an id outside the point
    table mark nothing (the reference raises KeyError); a failed solver comes back with success False and zeros and the vote over
    all matched ids (the reference fails at its own print of ret['num_inliers']); with an empty vote reference_frame_id stays the
    localisation's."""
    counts, dev, B, n_cov = _preamble(features, store, covisibility_frame)
    if B == 0:
        return []
    if image_sizes is None:
        if _pose.camera_form(cameras) == "resident":
            raise ValueError("refine_by_projection: image_sizes is needed when cameras is device_cameras' result")
        image_sizes = image_size_table(cameras)
    if not torch.is_tensor(image_sizes):
        image_sizes = torch.from_numpy(np.ascontiguousarray(np.asarray(image_sizes, dtype=np.int32).reshape(-1, 2)))
    image_sizes = image_sizes.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(image_sizes.shape) != (B, 2):
        raise ValueError("image_sizes: expected one (width, height) per query")
    tables = store.point_tables(dev)
    if int(tables["n_points"]) < 1:
        return [None] * B      # a map without points: nothing to project
    enable = _device_enable(enable, B, dev)
    cams = _pose._device_cameras(cameras, dev)
    chosen, loc = state["chosen"], state["est"]
    cap = max(1, min(int(tables["n_points"]), (n_cov + 1) * store.max_frame_rows))
    bitmap, ref_frame = ops.projref_mark(chosen, state["plan"], tables, n_cov, enable)
    cand_pt, cand_uv, n_union, n_cand = ops.projref_project(bitmap, chosen, loc["qvec"].contiguous(), loc["tvec"].contiguous(), cams[0], cams[1],
                                                            image_sizes, tables, cap)
    kpts = features["keypoints"].contiguous()
    best, d0, d1, accept = ops.projref_match(kpts, features["descriptors"].contiguous(), counts.contiguous(), cand_pt, cand_uv, n_cand, tables,
                                             threshold)
    cor = ops.projref_correspond(accept, best, counts.contiguous(), kpts, cand_pt, n_cand, tables)
    dists = torch.stack([d0, d1], 2)
    own = lambda b, v: {"n_union": v["n_union"], "n_projected": v["n_projected"], "dists": dists[b, :max(0, min(v["n_query"], dists.shape[1]))]}
    return _solve_and_vote(cor, _PROJ_MATCHED, cams, store, tables, n_cov, ref_frame, {"n_union": n_union, "n_projected": n_cand, "n_query": counts}, own,
                           dict(threshold=threshold, trials=trials, min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed))


@torch.no_grad()
def localize_and_refine(features: dict, recognition, store, matcher, cameras, *, seg_k: int, min_kpts: int, threshold: float,
                        min_inliers: int, semantic_matching: bool = True, overlap_ratio: float = 0.5, trials: int = 1000,
                        min_inlier_ratio: float = 0.01, refine_iters: int = _pose.DEFAULT_REFINE_ITERS, seed: int = 0,
                        covisibility_frame: Optional[int] = None, enable=None, refinement_method: str = "matching",
                        projection_min_inliers: int = 64, image_sizes=None) -> List[dict]:
    """localize_candidates, then the refinement on its device-side state (do_refinement: true, multimap3d.py:245-271).
    refinement_method 'matching': refine_by_matching for every located query.  'projection': a query with tracking status True and
    num_inliers >= projection_min_inliers goes to refine_by_projection, every other located query to refine_by_matching
    (multimap3d.py:245-255); the two groups are the two functions' enable masks, built from what the localisation read back, and
    a function whose group is empty is not called.  Any other value: NotImplementedError (singlemap3d.py:266).
    -> per query localize_candidates' dict plus ``refinement``: the refining function's dict with ``method`` ('matching' or
    'projection'), or None for a query that was not refined; the localisation's entries are left as they are (a failed refinement
    changes nothing).  Host synchronisations: two for the localisation, two for the matching form, one for the projection form."""
    if refinement_method not in ("matching", "projection"):
        raise NotImplementedError(f"refinement_method {refinement_method!r}")
    out, state = _pose._localize(features, recognition, store, matcher, cameras, seg_k=seg_k, min_kpts=min_kpts, threshold=threshold,
                                 min_inliers=min_inliers, semantic_matching=semantic_matching, overlap_ratio=overlap_ratio, trials=trials,
                                 min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed)
    kw = dict(threshold=threshold, covisibility_frame=covisibility_frame, trials=trials, min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters,
              seed=seed)
    if refinement_method == "matching":
        ref = refine_by_matching(features, state, store, matcher, cameras, enable=enable, **kw)
        for r, x in zip(out, ref):
            if x is not None:
                x["method"] = "matching"
            r["refinement"] = x
        return out
    B = len(out)
    on = np.ones(B, dtype=bool) if enable is None else enable_mask(enable, B, bool)
    located = np.array([r["success"] for r in out], dtype=bool)
    strong = np.array([bool(r["tracking_status"]) and r["num_inliers"] >= projection_min_inliers for r in out], dtype=bool)
    by_proj, by_match = on & located & strong, on & located & ~strong
    ref: List[Optional[dict]] = [None] * B
    for mask, name, run in ((by_proj, "projection", lambda m: refine_by_projection(features, state, store, cameras, enable=m, image_sizes=image_sizes, **kw)),
                            (by_match, "matching", lambda m: refine_by_matching(features, state, store, matcher, cameras, enable=m, **kw))):
        if not mask.any():
            continue
        for b, x in enumerate(run(mask.astype(np.int32))):
            if x is not None and mask[b]:
                x["method"] = name
                ref[b] = x
    for r, x in zip(out, ref):
        r["refinement"] = x
    return out
