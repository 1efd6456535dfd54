"""Pose refinement by matching over covisible frames, on the device.

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

from typing import List, Optional

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import candidates as _cand
from pram_amd.localization import pose as _pose

_MATCHED = ("matched_keypoints", "matched_keypoint_ids", "matched_xyzs", "matched_point3D_ids", "matched_sids", "matched_ref_keypoints",
            "matched_src")


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
    counts = features["counts"]
    ops._chk(counts, "counts", torch.int32)
    dev, B = counts.device, counts.numel()
    n_cov = int(store.covisibility_frame if covisibility_frame is None else covisibility_frame)
    if n_cov < 1:
        raise ValueError("covisibility_frame < 1")
    if B == 0:
        return []
    tables = store.tables(dev)
    seg_k = int(state["seg_k"])
    if enable is not None:
        enable = torch.as_tensor(np.asarray(enable.cpu() if torch.is_tensor(enable) else enable).astype(np.int32).reshape(-1)).to(dev)
        if enable.numel() != B:
            raise ValueError("enable: expected one entry per query")
    chosen = state["chosen"]
    plan, ref_frame, used, init_on = ops.refine_plan(chosen, state["plan"], counts.contiguous(), tables, n_cov, enable)
    cor, host, m = _cand._match_planned(features, {"plan": plan, "vote": {"tokens": state["tokens"]}}, store, matcher)
    merged = ops.refine_merge(cor, state["cor"], chosen, init_on, n_cov)
    est = _pose.estimate_poses(merged["matched_keypoints"], merged["matched_xyzs"], merged["count"], cameras, seg_k=1, threshold=threshold,
                               trials=trials, min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed)
    k = max(1, min(n_cov, store.n_frames))
    best_f, _, n_best = ops.refine_frame_vote(merged["matched_point3D_ids"], merged["count"], est["inliers"], est["success"], tables, k)
    # the one read-back: 7 doubles and 7 + k ints per query
    ints = torch.stack([est["success"], est["num_inliers"], merged["count"], ref_frame, used, init_on, n_best], 1)
    packed = torch.cat([est["qvec"], est["tvec"], ints.double(), best_f.double()], 1).cpu().numpy()
    f = ops.CAND_PLAN_FIELDS
    col = lambda name: host[f.index(name)]
    out: List[Optional[dict]] = []
    for b in range(B):
        succ, ninl, n, rf, nu, ini, nb = (int(v) for v in packed[b, 7:14])
        if rf < 0:
            out.append(None)
            continue
        frames = [store.frame_ids[int(i)] for i in packed[b, 14:14 + nb]]
        r = {"success": bool(succ), "qvec": packed[b, :4].copy(), "tvec": packed[b, 4:7].copy(), "num_inliers": ninl,
             "inliers": est["inliers"][b, :n].bool(), "refinement_reference_frame_ids": frames,
             "reference_frame_id": frames[0] if frames else store.frame_ids[rf], "n_covisible": nu, "used_init": bool(ini)}
        r.update({key: merged[key][b, :n] for key in _MATCHED})
        slots = []
        for j in range(nu):
            p = b * n_cov + j
            l0 = int(col("lens0")[p])
            slots.append({"reference_frame_id": store.frame_ids[int(col("frame")[p])], "n_query_kpts": l0, "n_ref_kpts": int(col("lens1")[p]),
                          "matches0": m["matches0"][p, :l0], "matching_scores0": m["matching_scores0"][p, :l0], "n_matches": cor["count"][p]})
        r["slots"] = slots
        out.append(r)
    return out


@torch.no_grad()
def localize_and_refine(features: dict, recognition, store, matcher, cameras, *, seg_k: int, min_kpts: int, threshold: float,
                        min_inliers: int, semantic_matching: bool = True, overlap_ratio: float = 0.5, trials: int = 1000,
                        min_inlier_ratio: float = 0.01, refine_iters: int = _pose.DEFAULT_REFINE_ITERS, seed: int = 0,
                        covisibility_frame: Optional[int] = None, enable=None) -> List[dict]:
    """localize_candidates, then refine_by_matching on its device-side state (do_refinement: true with refinement_method
    'matching', multimap3d.py:245-271).  -> per query localize_candidates' dict plus ``refinement``: refine_by_matching's dict, or
    None for a query that was not refined; the localisation's entries are left as they are (a failed refinement changes nothing).
    Four host synchronisations in all: two per stage."""
    out, state = _pose._localize(features, recognition, store, matcher, cameras, seg_k=seg_k, min_kpts=min_kpts, threshold=threshold,
                                 min_inliers=min_inliers, semantic_matching=semantic_matching, overlap_ratio=overlap_ratio, trials=trials,
                                 min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed)
    ref = refine_by_matching(features, state, store, matcher, cameras, threshold=threshold, covisibility_frame=covisibility_frame, trials=trials,
                             min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed, enable=enable)
    for r, x in zip(out, ref):
        r["refinement"] = x
    return out
