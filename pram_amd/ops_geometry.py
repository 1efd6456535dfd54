"""Torch-facing wrappers over the localisation and mapping entries of the C ABI (include/pram_hip.h): candidates, pose, refinement,
tracking, the query pre-filter, map building and compression, k-means, triangulation, two-view geometry, outlier removal, retrieval,
bundle adjustment, incremental mapping and image retrieval.  They hold no state; pram_amd.ops re-exports every name here, and the
network hot path with the workspace cache stays there.  Five helpers carry what every wrapper does: _check (arguments), _new
(outputs), _ws (workspaces), _int_table (host tables) and _call (the entry)."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib

_INT64 = torch.int64


def _check(*items):
    """Every item (tensor, name, dtype[, min_numel]): on the device with that dtype (PramHipError), contiguous, and holding
    min_numel elements at least (AssertionError)."""
    for it in items:
        _chk(it[0], it[1], it[2])
        assert it[0].is_contiguous(), it[1]
        assert len(it) < 4 or it[0].numel() >= it[3], it[1]


def _new(dev, dtype, n: int, *rest) -> torch.Tensor:
    """An uninitialised output of max(n, 1) rows: an empty tensor has no storage to hand to an entry.  The caller cuts it to [:n]
    where it returns n rows."""
    return torch.empty(max(n, 1), *rest, device=dev, dtype=dtype)


def _ws(need: int, workspace: Optional[torch.Tensor], device, refusal: Optional[str] = None, floor: int = 0) -> torch.Tensor:
    """need: what the entry's *_workspace_bytes returned (with ``refusal``: 0 says it refuses the sizes) -> ``workspace`` checked,
    or a new one of max(need, floor) bytes."""
    if refusal is not None and need == 0:
        raise _lib.PramHipError(refusal)
    if workspace is None:
        return torch.empty(max(need, floor), device=device, dtype=torch.uint8)
    _chk(workspace, "workspace", torch.uint8)
    return workspace


def _int_table(a, refusal: Optional[str] = None):
    """A host table (what the entries validate) as a ctypes int array that is never empty behind its pointer, and its length;
    with ``refusal`` an empty table raises it."""
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32)
    if refusal is not None and a.size < 1:
        raise _lib.PramHipError(refusal)
    return (ctypes.c_int * max(a.size, 1)).from_buffer_copy(a.tobytes() if a.size else b"\0\0\0\0"), a.size


def _call(entry: str, *args, stream: Optional[int] = None):
    """The entry on the current stream (or on ``stream``, for a caller that launches in a loop): a tensor goes as its data pointer,
    None and numbers as they are; a return code other than 0 raises PramHipError under the entry's name."""
    _lib.check(getattr(_lib.load(), entry)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                                           _st() if stream is None else stream), entry)


# ---- candidate-landmark matching (csrc/candidates.hip; pram_amd/localization/candidates.py drives these) -------------------
CAND_PLAN_COLS = 10      # PRAM_CAND_PLAN_COLS
CAND_PLAN_FIELDS = ("query", "sid", "frame", "semantic", "lens0", "lens1", "tok_off", "row0", "sel_off", "order")


def seg_vote_batched(sorted_vals: torch.Tensor, sorted_ids: torch.Tensor, topk: int):
    """pram_seg_vote for a batch of queries ([B, N, C] sorted class lists): one launch per query into slices of batched buffers
    -> (win_sid [B, topk], win_rank, win_count, n_win [B], tokens [B, topk, N], mean_score [B, topk]), all on the device."""
    _check((sorted_vals, "sorted_vals", torch.float32), (sorted_ids, "sorted_ids", _INT64))
    assert sorted_vals.dim() == 3 and sorted_ids.shape == sorted_vals.shape
    B, n, c = sorted_vals.shape
    dev = sorted_vals.device
    topk = int(topk)
    sid, rank, cnt = _filled((B, topk), dev, torch.int32), _filled((B, topk), dev, torch.int32), _filled((B, topk), dev, torch.int32)
    nwin = _filled((B,), dev, torch.int32)
    tokens = _filled((B, topk, max(n, 1)), dev, torch.int32)
    mean = _filled((B, topk), dev)
    st = _st()
    for b in range(B if n else 0):      # n == 0: no tokens, no winners (the zero fill above)
        _call("pram_seg_vote", sorted_ids[b], sorted_vals[b], n, c, topk, sid[b], rank[b], cnt[b], nwin[b:], tokens[b], mean[b], stream=st)
    return sid, rank, cnt, nwin, tokens, mean


def cand_mask_ranks_(sorted_ids: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """In place: the sorted class ids [B, N, C] of the padded tokens (t >= counts[b]) become 0 (background) at every rank."""
    _check((sorted_ids, "sorted_ids", _INT64), (counts, "counts", torch.int32))
    assert sorted_ids.dim() == 3 and counts.numel() == sorted_ids.shape[0]
    B, n, c = sorted_ids.shape
    _call("pram_cand_mask_ranks", sorted_ids, counts, B, n, c)
    return sorted_ids


def cand_plan(win_sid, win_count, n_win, seg_ids, counts, n_class: int, store, min_kpts: int, overlap_ratio: float,
              semantic_matching: bool) -> torch.Tensor:
    """-> plan int32 [CAND_PLAN_COLS, B * seg_k] (one contiguous column per CAND_PLAN_FIELDS entry).  ``store``: the device tables
    of a ReferenceStore (dict of tensors: pram_cand_plan) or of a MultiMapStore (they carry lm_start: pram_cand_plan_maps)."""
    _check(*[(t, nm, torch.int32) for t, nm in ((win_sid, "win_sid"), (win_count, "win_count"), (n_win, "n_win"), (seg_ids, "seg_ids"),
                                                (counts, "counts"))])
    B, seg_k = win_sid.shape
    n = seg_ids.shape[1]
    assert seg_ids.shape[0] == B and counts.numel() == B and n_win.numel() == B and win_count.shape == win_sid.shape
    plan = torch.empty(CAND_PLAN_COLS, B * seg_k, device=win_sid.device, dtype=torch.int32)
    s = store
    maps = "lm_start" in s      # a MultiMapStore's tables: the landmark tables are indexed by the global id
    _call("pram_cand_plan_maps" if maps else "pram_cand_plan", win_sid, win_count, n_win, seg_ids, counts, B, n, int(n_class), seg_k, s["lm_frame"],
          s["lm_sel_off"], s["lm_sel_len"], int(s["n_landmarks"]), s["lm_start"] if maps else int(s["start_sid"]), s["frame_off"], s["hist_off"],
          s["hist_label"], s["hist_cnt"], int(s["n_frames"]), int(min_kpts), float(overlap_ratio), int(bool(semantic_matching)), plan)
    return plan


def cand_gather(plan: torch.Tensor, tokens: torch.Tensor, store, q_desc, q_kpts, q_scores, q_norm, t_pad: int):
    """-> dict(descriptors0/1 [P, T, 128], norm_keypoints0/1 [P, T, 2], scores0/1 [P, T]) filled from the plan; q_norm = (cx, cy, scale)
    of the queries' camera.  The two sides of each output are halves of one [2P, ...] buffer."""
    _check((q_desc, "descriptors", torch.float32), (q_kpts, "keypoints", torch.float32), (q_scores, "scores", torch.float32))
    B, n, D = q_desc.shape
    assert D == 128 and tuple(q_kpts.shape) == (B, n, 2) and tuple(q_scores.shape) == (B, n)
    P, T, dev = plan.shape[1], int(t_pad), q_desc.device
    d = torch.empty(2 * P, T, 128, device=dev, dtype=torch.float32)
    k = torch.empty(2 * P, T, 2, device=dev, dtype=torch.float32)
    sc = torch.empty(2 * P, T, device=dev, dtype=torch.float32)
    s = store
    _call("pram_cand_gather", plan, tokens, s["sel_rows"], q_desc, q_kpts, q_scores, n, s["descriptors"], s["keypoints"], s["scores"],
          s["frame_norm"], int(s["n_rows"]), float(q_norm[0]), float(q_norm[1]), float(q_norm[2]), d[:P], k[:P], sc[:P], d[P:], k[P:], sc[P:], P, T)
    return {"descriptors0": d[:P], "descriptors1": d[P:], "norm_keypoints0": k[:P], "norm_keypoints1": k[P:], "scores0": sc[:P], "scores1": sc[P:]}


# The match list every stage hands on: parallel tensors [P, cap] + tail with count int32 [P].  Key -> (dtype, tail), in the order
# the entries of pram_hip.h take the pointers.
MATCH_LIST = {"matched_keypoint_ids": (_INT64, ()), "matched_keypoints": (torch.float32, (2,)), "matched_ref_keypoints": (torch.float32, (2,)),
              "matched_point3D_ids": (_INT64, ()), "matched_xyzs": (torch.float64, (3,)), "matched_sids": (torch.int32, ())}
MATCH_KEYS = tuple(MATCH_LIST)
MATCH_REF_KPTS, MATCH_SRC = "matched_ref_keypoints", "matched_src"      # the list projref_correspond leaves out, the one refine_merge adds
MATCH_NOREF_KEYS = tuple(k for k in MATCH_KEYS if k != MATCH_REF_KPTS)
MATCH_POINT_KEYS = tuple(k for k in MATCH_NOREF_KEYS if k != "matched_keypoints")      # the four lists update_point3ds reads
# the order the result dicts of localization/ list them in (the reference's)
MATCH_RESULT_KEYS = tuple(MATCH_KEYS[i] for i in (1, 0, 4, 3, 5, 2))


def _cor_chk(cor: dict, name: str, keys=MATCH_KEYS, src: bool = False):
    """dtypes, contiguity and shapes of the lists ``keys`` of cor (src: and of matched_src) and of its count -> (P, cap)."""
    P, t = cor["matched_keypoint_ids"].shape
    for k in keys + ((MATCH_SRC,) if src else ()):
        dt, tail = MATCH_LIST.get(k, (torch.int32, ()))
        _check((cor[k], f"{name}.{k}", dt))
        assert tuple(cor[k].shape) == (P, t) + tail, (name, k)
    _check((cor["count"], f"{name}.count", torch.int32))
    assert cor["count"].numel() == P
    return P, t


def _cor_alloc(B: int, cap: int, dev, keys=MATCH_KEYS, src: bool = False) -> dict:
    """Uninitialised lists ``keys`` [B, max(cap, 1)] (src: and matched_src), then count."""
    c1 = max(int(cap), 1)
    out = {k: torch.empty((B, c1) + MATCH_LIST[k][1], device=dev, dtype=MATCH_LIST[k][0]) for k in keys}
    if src:
        out[MATCH_SRC] = torch.empty(B, c1, device=dev, dtype=torch.int32)
    out["count"] = torch.empty(B, device=dev, dtype=torch.int32)
    return out


def cand_correspond(matches0: torch.Tensor, plan: torch.Tensor, tokens: torch.Tensor, store, q_kpts: torch.Tensor, cap: int):
    """matches0 int64 [P, >= T0] -> dict of padded per-pair outputs [P, cap, ...] and count int32 [P] (pram_cand_correspond)."""
    _chk(matches0, "matches0", _INT64)
    _check((q_kpts, "keypoints", torch.float32))
    assert matches0.dim() == 2 and matches0.stride(1) == 1
    P, t0 = matches0.shape
    assert plan.shape[1] == P
    n, cap = q_kpts.shape[1], int(cap)
    out = _cor_alloc(P, cap, matches0.device)
    s = store
    _call("pram_cand_correspond", matches0, matches0.stride(0), plan, tokens, s["sel_rows"], q_kpts, n, s["keypoints"], s["xyzs"], s["point3D_ids"],
          s["keypoint_segs"], int(s["n_rows"]), P, t0, cap, *[out[k] for k in MATCH_KEYS], out["count"])
    return out


# ---- batched absolute pose (csrc/pose.hip; pram_amd/localization/pose.py drives these) ---------------------------------------
CAMERA_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4}      # PRAM_CAM_*
POSE_CAM_PARAMS = 8      # PRAM_POSE_CAM_PARAMS


def _pose_chk(m_kpts, m_xyz, counts):
    _check((m_kpts, "matched_keypoints", torch.float32), (m_xyz, "matched_xyzs", torch.float64), (counts, "counts", torch.int32))
    P, t0 = m_kpts.shape[:2]
    assert tuple(m_kpts.shape) == (P, t0, 2) and tuple(m_xyz.shape) == (P, t0, 3) and counts.numel() == P
    return P, t0


def _pose_chk_stage(norm_pts, m_xyz, counts, cam_model, cam_params, seg_k):
    """dtype, device, contiguity and shapes of what pose_score / pose_refine hand over as raw pointers -> (P, t0, B)."""
    _check((norm_pts, "norm_pts", torch.float64), (m_xyz, "matched_xyzs", torch.float64), (counts, "counts", torch.int32),
           (cam_model, "cam_model", torch.int32), (cam_params, "cam_params", torch.float64))
    P, t0 = norm_pts.shape[:2]
    B, seg_k = cam_model.numel(), int(seg_k)
    assert tuple(norm_pts.shape) == (P, t0, 2) and tuple(m_xyz.shape) == (P, t0, 3) and counts.numel() == P
    assert seg_k >= 1 and P == B * seg_k and tuple(cam_params.shape) == (B, POSE_CAM_PARAMS)
    return P, t0, B


def pose_prepare(m_kpts: torch.Tensor, counts: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor, cam_model_host,
                 seg_k: int) -> torch.Tensor:
    """matched_keypoints float32 [P, t0, 2] (+ 0.5 inside) -> normalised camera-plane points float64 [P, t0, 2]; rows >= counts[p]
    are left unwritten.  cam_model int32 [B], cam_params float64 [B, 8] on the device, cam_model_host: the ids on the host
    (a sequence of ints), which is what the launcher validates."""
    _check((m_kpts, "matched_keypoints", torch.float32), (counts, "counts", torch.int32), (cam_model, "cam_model", torch.int32),
           (cam_params, "cam_params", torch.float64))
    P, t0 = m_kpts.shape[:2]
    B, seg_k = cam_model.numel(), int(seg_k)
    assert seg_k >= 1 and P == B * seg_k and counts.numel() == P and tuple(cam_params.shape) == (B, POSE_CAM_PARAMS) and len(cam_model_host) == B
    host, _ = _int_table(cam_model_host)
    pts = torch.empty(P, t0, 2, device=m_kpts.device, dtype=torch.float64)
    _call("pram_pose_prepare", m_kpts, counts, cam_model, cam_params, ctypes.addressof(host), B, seg_k, t0, pts)
    return pts


def pose_hypotheses(norm_pts: torch.Tensor, m_xyz: torch.Tensor, counts: torch.Tensor, trials: int, seed: int, with_triples: bool = False):
    """-> (poses float64 [P, trials, 4, 12], n_sol int32 [P, trials][, triples int32 [P, trials, 3]])."""
    _check((norm_pts, "norm_pts", torch.float64), (m_xyz, "matched_xyzs", torch.float64), (counts, "counts", torch.int32))
    P, t0 = norm_pts.shape[:2]
    assert tuple(m_xyz.shape) == (P, t0, 3) and counts.numel() == P
    trials, dev = int(trials), norm_pts.device
    poses = torch.empty(P, max(trials, 1), 4, 12, device=dev, dtype=torch.float64)
    n_sol = torch.empty(P, max(trials, 1), device=dev, dtype=torch.int32)
    tri = torch.empty(P, max(trials, 1), 3, device=dev, dtype=torch.int32) if with_triples else None
    _call("pram_pose_hypotheses", norm_pts, m_xyz, counts, P, t0, trials, int(seed) & 0xFFFFFFFFFFFFFFFF, poses, n_sol, tri)
    return (poses, n_sol, tri) if with_triples else (poses, n_sol)


def pose_score(norm_pts, m_xyz, counts, poses, n_sol, cam_model, cam_params, seg_k: int, threshold: float):
    """-> (h_inliers int32 [P, trials * 4] (-1 = empty slot), h_resid float64 [P, trials * 4], best int32 [P])."""
    P, t0, B = _pose_chk_stage(norm_pts, m_xyz, counts, cam_model, cam_params, seg_k)
    trials, dev = poses.shape[1], norm_pts.device
    _check((poses, "poses", torch.float64), (n_sol, "n_sol", torch.int32))
    assert tuple(poses.shape) == (P, trials, 4, 12) and tuple(n_sol.shape) == (P, trials)
    h_inl = torch.empty(P, trials * 4, device=dev, dtype=torch.int32)
    h_res = torch.empty(P, trials * 4, device=dev, dtype=torch.float64)
    best = torch.empty(P, device=dev, dtype=torch.int32)
    _call("pram_pose_score", norm_pts, m_xyz, counts, poses, n_sol, cam_model, cam_params, P, int(seg_k), t0, trials, float(threshold), h_inl, h_res,
          best)
    return h_inl, h_res, best


def pose_refine(m_kpts, norm_pts, m_xyz, counts, poses, h_inl, best, cam_model, cam_params, seg_k: int, threshold: float,
                min_inlier_ratio: float, refine_iters: int) -> dict:
    """-> dict(qvec float64 [P, 4] (w, x, y, z), tvec [P, 3], inliers uint8 [P, t0], num_inliers int32 [P], success int32 [P])."""
    P, t0 = _pose_chk(m_kpts, m_xyz, counts)
    _pose_chk_stage(norm_pts, m_xyz, counts, cam_model, cam_params, seg_k)
    trials, dev = poses.shape[1], m_kpts.device
    _check((poses, "poses", torch.float64), (h_inl, "h_inliers", torch.int32), (best, "best", torch.int32))
    assert tuple(poses.shape) == (P, trials, 4, 12) and tuple(h_inl.shape) == (P, trials * 4) and best.numel() == P
    out = {"qvec": torch.empty(P, 4, device=dev, dtype=torch.float64), "tvec": torch.empty(P, 3, device=dev, dtype=torch.float64),
           "inliers": torch.empty(P, t0, device=dev, dtype=torch.uint8), "num_inliers": torch.empty(P, device=dev, dtype=torch.int32),
           "success": torch.empty(P, device=dev, dtype=torch.int32)}
    _call("pram_pose_refine", m_kpts, norm_pts, m_xyz, counts, poses, h_inl, best, cam_model, cam_params, P, int(seg_k), t0, trials, float(threshold),
          float(min_inlier_ratio), int(refine_iters), out["qvec"], out["tvec"], out["inliers"], out["num_inliers"], out["success"])
    return out


def pose_select(success: torch.Tensor, num_inliers: torch.Tensor, seg_k: int, min_inliers: int) -> torch.Tensor:
    """success / num_inliers int32 [B * seg_k] -> int32 [B, 3]: kept candidate (-1 none), tracking status (1 / 0 / -1 none), order."""
    _check((success, "success", torch.int32), (num_inliers, "num_inliers", torch.int32))
    seg_k = int(seg_k)
    assert success.numel() == num_inliers.numel()
    assert seg_k >= 1 and success.numel() % seg_k == 0
    B = success.numel() // seg_k
    chosen = torch.empty(B, 3, device=success.device, dtype=torch.int32)
    _call("pram_pose_select", success, num_inliers, B, seg_k, int(min_inliers), chosen)
    return chosen


# ---- pose refinement by matching over covisible frames (csrc/refine.hip; pram_amd/localization/refine.py drives these) ---------
def refine_plan(chosen: torch.Tensor, loc_plan: torch.Tensor, counts: torch.Tensor, store, n_cov: int, enable: Optional[torch.Tensor] = None):
    """chosen int32 [B, 3] (pose_select), loc_plan int32 [CAND_PLAN_COLS, B * seg_k], counts int32 [B], ``store``: the device tables
    of a ReferenceStore -> (plan int32 [CAND_PLAN_COLS, B * n_cov], ref_frame, n_cov_used, init_on int32 [B])."""
    _check((chosen, "chosen", torch.int32), (loc_plan, "plan", torch.int32), (counts, "counts", torch.int32),
           *(((enable, "enable", torch.int32),) if enable is not None else ()))
    B, n_cov = counts.numel(), int(n_cov)
    assert tuple(chosen.shape) == (B, 3) and loc_plan.dim() == 2 and loc_plan.shape[0] == CAND_PLAN_COLS and (enable is None or enable.numel() == B)
    seg_k = loc_plan.shape[1] // B if B else 1
    assert seg_k >= 1 and loc_plan.shape[1] == B * seg_k
    dev = counts.device
    plan = torch.empty(CAND_PLAN_COLS, B * max(n_cov, 0), device=dev, dtype=torch.int32)
    ref_frame, used, init_on = (torch.empty(B, device=dev, dtype=torch.int32) for _ in range(3))
    s = store
    _call("pram_refine_plan", chosen, loc_plan, counts, enable, s["frame_off"], s["covis_off"], s["covis_frames"], B, seg_k, n_cov, int(s["n_frames"]),
          int(s["n_covis"]), plan, ref_frame, used, init_on)
    return plan, ref_frame, used, init_on


def refine_merge(cor_ref: dict, cor_loc: dict, chosen: torch.Tensor, init_on: torch.Tensor, n_cov: int, out: Optional[dict] = None) -> dict:
    """cor_ref / cor_loc: cand_correspond's dicts for the B * n_cov refinement pairs and the B * seg_k localisation pairs
    -> one list per query, dict of [B, cap, ...] tensors (cap = n_cov * t0 + t0a) with the keys of cand_correspond plus
    matched_src int32 and count int32 [B].  ``out``: buffers to write into (the tests pre-fill them)."""
    Pr, t0 = _cor_chk(cor_ref, "refinement")
    Pa, t0a = _cor_chk(cor_loc, "localisation")
    _check((chosen, "chosen", torch.int32), (init_on, "init_on", torch.int32))
    B, n_cov = init_on.numel(), int(n_cov)
    assert tuple(chosen.shape) == (B, 3) and Pr == B * n_cov
    seg_k = Pa // B if B else 1
    assert seg_k >= 1 and Pa == B * seg_k
    if out is None:
        out = _cor_alloc(B, n_cov * t0 + t0a, init_on.device, src=True)
    else:
        assert _cor_chk(out, "out", src=True)[0] == B
    cap = out["matched_sids"].shape[1]
    r, a, o = cor_ref, cor_loc, out
    _call("pram_refine_merge", *[r[k] for k in MATCH_KEYS], r["count"], t0, *[a[k] for k in MATCH_KEYS], a["count"], t0a, chosen, init_on, B, seg_k,
          n_cov, cap, *[o[k] for k in MATCH_KEYS], o[MATCH_SRC], o["count"])
    return out


def refine_frame_vote(m_point3d_ids: torch.Tensor, m_count: torch.Tensor, inliers: torch.Tensor, success: torch.Tensor, store, k: int):
    """find_reference_frames per query over the merged list -> (best_frames int32 [B, k] (store frame indices, -1 padded),
    best_counts int32 [B, k], n_best int32 [B])."""
    _check((m_point3d_ids, "matched_point3D_ids", _INT64), (m_count, "count", torch.int32), (inliers, "inliers", torch.uint8),
           (success, "success", torch.int32))
    B, cap = m_point3d_ids.shape
    assert tuple(inliers.shape) == (B, cap) and m_count.numel() == B and success.numel() == B
    dev, k, s = m_point3d_ids.device, int(k), store
    hist = torch.empty(B, max(int(s["n_frames"]), 1), device=dev, dtype=torch.int32)      # zeroed by the entry
    best_f, best_c = torch.empty(B, max(k, 1), device=dev, dtype=torch.int32), torch.empty(B, max(k, 1), device=dev, dtype=torch.int32)
    n_best = torch.empty(B, device=dev, dtype=torch.int32)
    _call("pram_refine_frame_vote", m_point3d_ids, m_count, inliers, success, B, cap, s["pt_ids"], s["pt_off"], s["pt_frames"], int(s["n_points"]),
          int(s["n_pt_entries"]), s["is_vrf"], int(s["n_frames"]), k, hist, best_f, best_c, n_best)
    return best_f, best_c, n_best


# ---- pose refinement by projection over covisible frames (csrc/projref.hip; pram_amd/localization/refine.py drives these) ------
def projref_mark(chosen: torch.Tensor, loc_plan: torch.Tensor, store, n_cov: int, enable: Optional[torch.Tensor] = None):
    """chosen int32 [B, 3], loc_plan int32 [CAND_PLAN_COLS, B * seg_k], ``store``: the device tables of a ReferenceStore
    -> (bitmap int32 [B, ceil(n_points / 32)] over the point table, ref_frame int32 [B])."""
    _check((chosen, "chosen", torch.int32), (loc_plan, "plan", torch.int32), *(((enable, "enable", torch.int32),) if enable is not None else ()))
    B, n_cov, s = chosen.shape[0], int(n_cov), store
    assert tuple(chosen.shape) == (B, 3) and loc_plan.dim() == 2 and loc_plan.shape[0] == CAND_PLAN_COLS and (enable is None or enable.numel() == B)
    seg_k = loc_plan.shape[1] // B if B else 1
    assert seg_k >= 1 and loc_plan.shape[1] == B * seg_k
    n_points, dev = int(s["n_points"]), chosen.device
    bitmap = torch.empty(B, max((n_points + 31) // 32, 1), device=dev, dtype=torch.int32)      # zeroed by the entry
    ref_frame = torch.empty(B, device=dev, dtype=torch.int32)
    _call("pram_projref_mark", chosen, loc_plan, enable, s["frame_off"], s["covis_off"], s["covis_frames"], s["point3D_ids"], s["pt_ids"], B, seg_k,
          n_cov, int(s["n_frames"]), int(s["n_covis"]), int(s["n_rows"]), n_points, bitmap, ref_frame)
    return bitmap, ref_frame


def projref_project(bitmap: torch.Tensor, chosen: torch.Tensor, qvec: torch.Tensor, tvec: torch.Tensor, cam_model: torch.Tensor,
                    cam_params: torch.Tensor, image_size: torch.Tensor, store, cap: int):
    """bitmap: projref_mark's; qvec float64 [B * seg_k, 4], tvec [B * seg_k, 3]; cam_model int32 [B], cam_params float64 [B, 8],
    image_size int32 [B, 2] (width, height); ``store``: ReferenceStore.point_tables
    -> (cand_pt int32 [B, cap], cand_uv float64 [B, 2, cap], n_union int32 [B], n_cand int32 [B])."""
    _check((bitmap, "bitmap", torch.int32), (chosen, "chosen", torch.int32), (qvec, "qvec", torch.float64), (tvec, "tvec", torch.float64),
           (cam_model, "cam_model", torch.int32), (cam_params, "cam_params", torch.float64), (image_size, "image_size", torch.int32))
    B, cap, s = chosen.shape[0], int(cap), store
    n_points = int(s["n_points"])
    seg_k = qvec.shape[0] // B if B else 1
    assert tuple(chosen.shape) == (B, 3) and seg_k >= 1 and tuple(qvec.shape) == (B * seg_k, 4) and tuple(tvec.shape) == (B * seg_k, 3)
    assert tuple(bitmap.shape) == (B, max((n_points + 31) // 32, 1)) and cam_model.numel() == B and tuple(cam_params.shape) == (B, POSE_CAM_PARAMS)
    assert tuple(image_size.shape) == (B, 2) and s["pt_xyz"].shape[0] >= n_points
    dev = chosen.device
    cand_pt = torch.empty(B, max(cap, 1), device=dev, dtype=torch.int32)
    cand_uv = torch.empty(B, 2, max(cap, 1), device=dev, dtype=torch.float64)
    n_union, n_cand = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    _call("pram_projref_project", bitmap, n_points, s["pt_xyz"], chosen, qvec, tvec, cam_model, cam_params, image_size, B, seg_k, cap, cand_pt, cand_uv,
          n_union, n_cand)
    return cand_pt, cand_uv, n_union, n_cand


def projref_match(q_kpts: torch.Tensor, q_desc: torch.Tensor, counts: torch.Tensor, cand_pt: torch.Tensor, cand_uv: torch.Tensor,
                  n_cand: torch.Tensor, store, threshold: float):
    """q_kpts [B, N, 2], q_desc [B, N, 128], counts int32 [B]; cand_*: projref_project's; ``store``: ReferenceStore.point_tables
    -> (best int32 [B, N] (candidate index, -1 none), d0, d1 float32 [B, N] (+inf: none), accept uint8 [B, N])."""
    _check((q_kpts, "keypoints", torch.float32), (q_desc, "descriptors", torch.float32), (counts, "counts", torch.int32),
           (cand_pt, "cand_pt", torch.int32), (cand_uv, "cand_uv", torch.float64), (n_cand, "n_cand", torch.int32))
    B, N, D = q_desc.shape
    cap, s = cand_pt.shape[1], store
    assert D == 128 and tuple(q_kpts.shape) == (B, N, 2) and counts.numel() == B and n_cand.numel() == B
    assert tuple(cand_pt.shape) == (B, cap) and tuple(cand_uv.shape) == (B, 2, cap) and s["pt_desc"].shape[0] >= int(s["n_points"])
    dev = q_desc.device
    best = torch.empty(B, max(N, 1), device=dev, dtype=torch.int32)[:, :N]
    d0, d1 = torch.empty(B, max(N, 1), device=dev)[:, :N], torch.empty(B, max(N, 1), device=dev)[:, :N]
    accept = torch.empty(B, max(N, 1), device=dev, dtype=torch.uint8)[:, :N]
    if N == 0:      # no keypoints: the empty inputs have no storage to hand to the entry
        return best, d0, d1, accept
    _call("pram_projref_match", q_kpts, q_desc, counts, B, N, cand_pt, cand_uv, n_cand, cap, s["pt_desc"], int(s["n_points"]), float(threshold), best,
          d0, d1, accept)
    return best, d0, d1, accept


def projref_correspond(accept: torch.Tensor, best: torch.Tensor, counts: torch.Tensor, q_kpts: torch.Tensor, cand_pt: torch.Tensor,
                       n_cand: torch.Tensor, store, out: Optional[dict] = None) -> dict:
    """-> pram_cand_correspond's layout with N rows per query: matched_keypoint_ids int64 [B, N], matched_keypoints [B, N, 2],
    matched_point3D_ids int64 [B, N], matched_xyzs float64 [B, N, 3], matched_sids int32 [B, N], count int32 [B].  ``out``: buffers
    to write into (the tests pre-fill them)."""
    _check((accept, "accept", torch.uint8), (best, "best", torch.int32), (counts, "counts", torch.int32), (q_kpts, "keypoints", torch.float32),
           (cand_pt, "cand_pt", torch.int32), (n_cand, "n_cand", torch.int32))
    B, N = accept.shape
    cap, s = cand_pt.shape[1], store
    assert tuple(best.shape) == (B, N) and tuple(q_kpts.shape) == (B, N, 2) and counts.numel() == B and n_cand.numel() == B and cand_pt.shape[0] == B
    if out is None:
        out = _cor_alloc(B, N, accept.device, MATCH_NOREF_KEYS)
    else:
        assert _cor_chk(out, "out", MATCH_NOREF_KEYS) == (B, max(N, 1))
    if N == 0:      # no keypoints: the empty inputs have no storage to hand to the entry
        out["count"].zero_()
        return out
    _call("pram_projref_correspond", accept, best, counts, q_kpts, B, N, cand_pt, n_cand, cap, s["pt_ids"], s["pt_xyz"], s["pt_sid"], int(s["n_points"]),
          *[out[k] for k in MATCH_NOREF_KEYS], out["count"])
    return out


# ---- tracking the last frame for a batch of streams (csrc/track.hip; pram_amd/localization/tracker.py drives these) ------------
def _track_state_chk(st: dict):
    """st: the arrays of a TrackState (dict: keypoints, scores, descriptors, counts, xyzs, point3D_ids, seg_ids, ref_frame,
    frame_norm, n_slots, n_max) -> (n_slots, n_max)."""
    S, n_max = int(st["n_slots"]), int(st["n_max"])
    for k, dt, shape in (("keypoints", torch.float32, (S, n_max, 2)), ("scores", torch.float32, (S, n_max)), ("descriptors", torch.float32, (S, n_max, 128)),
                         ("counts", torch.int32, (S,)), ("xyzs", torch.float64, (S, n_max, 3)), ("point3D_ids", _INT64, (S, n_max)),
                         ("seg_ids", torch.int32, (S, n_max)), ("ref_frame", torch.int32, (S,)), ("frame_norm", torch.float32, (S, 3))):
        _check((st[k], f"state.{k}", dt))
        assert tuple(st[k].shape) == shape, k
    return S, n_max


def track_plan(counts: torch.Tensor, slot: torch.Tensor, st: dict, n: int):
    """counts, slot int32 [B] -> (plan, loc_plan) int32 [CAND_PLAN_COLS, B] (pram_track_plan)."""
    S, n_max = _track_state_chk(st)
    _check((counts, "counts", torch.int32), (slot, "slot", torch.int32))
    B = counts.numel()
    assert slot.numel() == B
    plan = torch.empty(CAND_PLAN_COLS, B, device=counts.device, dtype=torch.int32)
    loc_plan = torch.empty(CAND_PLAN_COLS, B, device=counts.device, dtype=torch.int32)
    if B == 0:      # no queries: the empty tensors have no storage to hand to the entry
        return plan, loc_plan
    _call("pram_track_plan", counts, slot, st["counts"], st["ref_frame"], B, int(n), S, n_max, plan, loc_plan)
    return plan, loc_plan


def track_gather_tables(st: dict, dummy: torch.Tensor) -> dict:
    """The state's arrays under the names cand_gather reads from a ReferenceStore's tables (sel_rows: never read, sel offset -1)."""
    return {"sel_rows": dummy, "descriptors": st["descriptors"], "keypoints": st["keypoints"], "scores": st["scores"], "frame_norm": st["frame_norm"],
            "n_rows": int(st["n_slots"]) * int(st["n_max"])}


def track_correspond(matches0: torch.Tensor, plan: torch.Tensor, st: dict, q_kpts: torch.Tensor, cap: int, out: Optional[dict] = None) -> dict:
    """matches0 int64 [B, >= t0] -> cand_correspond's dict, [B, cap, ...] and count int32 [B] (pram_track_correspond).  ``out``:
    buffers to write into (the tests pre-fill them)."""
    S, n_max = _track_state_chk(st)
    _chk(matches0, "matches0", _INT64)
    _check((q_kpts, "keypoints", torch.float32), (plan, "plan", torch.int32))
    assert matches0.dim() == 2 and matches0.stride(1) == 1
    P, t0 = matches0.shape
    assert tuple(plan.shape) == (CAND_PLAN_COLS, P) and q_kpts.dim() == 3 and q_kpts.shape[0] == P
    n, cap = q_kpts.shape[1], int(cap)
    if out is None:
        out = _cor_alloc(P, cap, matches0.device)
    else:
        _cor_chk(out, "out")
        assert out["matched_sids"].shape[0] == P and out["matched_sids"].shape[1] >= cap
        cap = out["matched_sids"].shape[1]
    _call("pram_track_correspond", matches0, matches0.stride(0) if P else t0, plan, q_kpts, n, st["keypoints"], st["xyzs"], st["point3D_ids"],
          st["seg_ids"], S, n_max, P, t0, cap, *[out[k] for k in MATCH_KEYS], out["count"])
    return out


def track_filter(cor: dict, mask: torch.Tensor, out: Optional[dict] = None) -> dict:
    """cor: cand_correspond-shaped lists [B, cap, ...] with count; mask uint8 [B, cap] -> the rows r < count[b] with mask != 0, in
    order, in new buffers of the same layout (pram_track_filter)."""
    B, cap = _cor_chk(cor, "lists")
    _check((mask, "mask", torch.uint8))
    assert tuple(mask.shape) == (B, cap)
    if out is None:
        out = _cor_alloc(B, cap, mask.device)
    else:
        assert _cor_chk(out, "out") == (B, cap)
    _call("pram_track_filter", *[cor[k] for k in MATCH_KEYS], cor["count"], mask, B, cap, *[out[k] for k in MATCH_KEYS], out["count"])
    return out


def track_commit(st: dict, q_kpts: torch.Tensor, q_scores: torch.Tensor, q_desc: torch.Tensor, counts: torch.Tensor, seg_ids: Optional[torch.Tensor],
                 slot: torch.Tensor, slot_host, ref_frame: torch.Tensor, q_norm, cor: dict, mask: Optional[torch.Tensor] = None,
                 winner: Optional[torch.Tensor] = None) -> None:
    """In place on the state (pram_track_commit): the queries with slot >= 0 become their slots' last frames and the list rows of
    ``cor`` (with ``mask`` uint8 [B, cap]: those with mask != 0) give their keypoints a point.  slot_host: the slots on the host (a
    sequence of ints), which is what the launcher validates; q_norm = (cx, cy, scale) of the queries' camera."""
    S, n_max = _track_state_chk(st)
    _check((q_kpts, "keypoints", torch.float32), (q_scores, "scores", torch.float32), (q_desc, "descriptors", torch.float32),
           (counts, "counts", torch.int32), (slot, "slot", torch.int32), (ref_frame, "ref_frame", torch.int32),
           *(((seg_ids, "seg_ids", torch.int32),) if seg_ids is not None else ()), *(((mask, "mask", torch.uint8),) if mask is not None else ()))
    B, n, D = q_desc.shape
    Bc, cap = _cor_chk(cor, "lists", MATCH_POINT_KEYS)
    assert D == 128 and tuple(q_kpts.shape) == (B, n, 2) and tuple(q_scores.shape) == (B, n) and counts.numel() == B and slot.numel() == B
    assert ref_frame.numel() == B and len(slot_host) == B and Bc == B and (seg_ids is None or tuple(seg_ids.shape) == (B, n))
    assert mask is None or tuple(mask.shape) == (B, cap)
    if winner is None:
        winner = torch.empty(B, max(n, 1), device=q_desc.device, dtype=torch.int32)
    _check((winner, "winner", torch.int32, B * n))
    host, _ = _int_table(slot_host)
    _call("pram_track_commit", q_kpts, q_scores, q_desc, counts, seg_ids, slot, ctypes.addressof(host), ref_frame, B, n, float(q_norm[0]),
          float(q_norm[1]), float(q_norm[2]), *[cor[k] for k in MATCH_POINT_KEYS], cor["count"], mask, cap, st["keypoints"], st["scores"],
          st["descriptors"], st["counts"], st["xyzs"], st["point3D_ids"], st["seg_ids"], st["ref_frame"], st["frame_norm"], S, n_max, winner)


# ---- the query pre-filter (csrc/prefilter.hip; pram_amd/localization/localizer.py drives it) -------------------------------------
def query_prefilter(keypoints: torch.Tensor, scores: torch.Tensor, descriptors: torch.Tensor, logits: torch.Tensor, seg_ids: torch.Tensor,
                    non_bg_mask: torch.Tensor, n_non_bg: torch.Tensor, counts: torch.Tensor, enable: bool) -> dict:
    """Frame.add_segmentations' filtering of the query for a padded batch (pram_query_prefilter).  keypoints [B, N, 2], scores
    [B, N], descriptors [B, N, D], logits [B, N, C] float32; seg_ids, non_bg_mask [B, N], n_non_bg [B] int32 = seg_epilogue's
    outputs at the filtering threshold; counts [B] int32; enable = the threshold is > 0.  -> dict(keypoints, scores, descriptors,
    logits, seg_ids: new buffers of the same shapes, compacted; counts [B]; kept int32 [B, N]; filtered int32 [B]).  No read-back."""
    _check((keypoints, "keypoints", torch.float32), (scores, "scores", torch.float32), (descriptors, "descriptors", torch.float32),
           (logits, "logits", torch.float32), (seg_ids, "seg_ids", torch.int32), (non_bg_mask, "non_bg_mask", torch.int32),
           (n_non_bg, "n_non_bg", torch.int32), (counts, "counts", torch.int32))
    assert descriptors.dim() == 3 and logits.dim() == 3
    B, N, D = descriptors.shape
    Cc = logits.shape[2]
    assert tuple(keypoints.shape) == (B, N, 2) and tuple(scores.shape) == (B, N) and tuple(logits.shape[:2]) == (B, N)
    assert tuple(seg_ids.shape) == (B, N) and tuple(non_bg_mask.shape) == (B, N) and n_non_bg.numel() == B and counts.numel() == B
    dev = descriptors.device
    out = {"keypoints": torch.empty_like(keypoints), "scores": torch.empty_like(scores), "descriptors": torch.empty_like(descriptors),
           "logits": torch.empty_like(logits), "seg_ids": torch.empty_like(seg_ids), "kept": torch.empty((B, N), device=dev, dtype=torch.int32)}
    if B == 0 or N == 0:      # the empty tensors have no storage to hand to the entry; an empty query keeps nothing, and fires
        out["counts"], out["filtered"] = _filled((B,), dev, torch.int32), _filled((B,), dev, torch.int32, 1 if enable else 0)      # (0 >= 0.4 * 0)
        return out
    out["counts"], out["filtered"] = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    _call("pram_query_prefilter", keypoints, scores, descriptors, logits, seg_ids, non_bg_mask, n_non_bg, counts, 1 if enable else 0, B, N, Cc, D,
          out["keypoints"], out["scores"], out["descriptors"], out["logits"], out["seg_ids"], out["counts"], out["kept"], out["filtered"])
    return out


# ---- map building (csrc/mapbuild.hip; pram_amd/localization/mapbuild.py drives these) ------------------------------------------
MAPBUILD_SHORT_TRACK, MAPBUILD_ROW_LDS, MAPBUILD_MAX_VRF, MAPBUILD_CAM_COLS = 32, 512, 64, 13      # include/pram_hip.h


def mapbuild_assign_descriptors(store, trk_off: torch.Tensor, trk_off_host, trk_frame: torch.Tensor, trk_kpt: torch.Tensor,
                                workspace: Optional[torch.Tensor] = None):
    """``store``: the device tables of a ReferenceStore; the tracks as CSR, trk_off int32 [P + 1] with its host copy, trk_frame /
    trk_kpt int32 [E] (store frame index or -1, keypoint index inside the frame) -> (pt_desc float32 [P, 128], pt_choice int32 [P]:
    the position of the chosen entry in the track, -1 for a track with nothing kept).  ``workspace``: uint8, at least
    pram_mapbuild_desc_workspace_bytes; None allocates it."""
    s = store
    host, P = _int_table(trk_off_host, "trk_off: an offset table has at least one entry")
    P -= 1
    E = int(host[P])
    _check((trk_off, "trk_off", torch.int32, P + 1), (trk_frame, "trk_frame", torch.int32, E), (trk_kpt, "trk_kpt", torch.int32, E),
           (s["descriptors"], "descriptors", torch.float32))
    assert s["descriptors"].shape[-1] == 128
    dev = trk_off.device
    workspace = _ws(int(_lib.load().pram_mapbuild_desc_workspace_bytes(ctypes.addressof(host), P)), workspace, dev, floor=8)
    pt_desc, pt_choice = _new(dev, torch.float32, P, 128), _new(dev, torch.int32, P)
    _call("pram_mapbuild_assign_descriptors", s["descriptors"], s["frame_off"], int(s["n_frames"]), int(s["n_rows"]), trk_off, ctypes.addressof(host),
          trk_frame, trk_kpt, P, workspace, workspace.numel(), pt_desc, pt_choice)
    return pt_desc[:P], pt_choice[:P]


def mapbuild_select_frames(store, pt_xyz: torch.Tensor, lm_off: torch.Tensor, lm_off_host, lm_points: torch.Tensor, frame_ignored: torch.Tensor,
                           frame_cams: torch.Tensor, min_obs: int = 120, topk_imgs: int = 500, n_vrf: int = 10, min_cover_ratio: float = 0.9,
                           gain_floor: float = 0.01, workspace: Optional[torch.Tensor] = None):
    """``store``: the device tables of a ReferenceStore (rows and point table); pt_xyz float64 [n_points, 3] aligned with pt_ids; the
    landmarks as CSR, lm_off int32 [L + 1] with its host copy and lm_points int64 [sum]; frame_ignored int32 [F]; frame_cams float64
    [F, MAPBUILD_CAM_COLS] (qvec, tvec, fx, fy, cx, cy, width, height) -> (lm_vrf int32 [L, n_vrf] store frame indices padded with
    -1, lm_vrf_n int32 [L]).  ``workspace``: uint8, at least pram_mapbuild_vrf_workspace_bytes; None allocates it."""
    s = store
    host, n_lm = _int_table(lm_off_host, "lm_off: an offset table has at least one entry")
    n_lm -= 1
    total = int(host[n_lm])
    F, n_points, n_vrf = int(s["n_frames"]), int(s["n_points"]), int(n_vrf)
    _check((pt_xyz, "pt_xyz", torch.float64, 3 * n_points), (lm_off, "lm_off", torch.int32, n_lm + 1), (lm_points, "lm_points", _INT64, total),
           (frame_ignored, "frame_ignored", torch.int32, F), (frame_cams, "frame_cams", torch.float64, F * MAPBUILD_CAM_COLS))
    dev = lm_off.device
    workspace = _ws(int(_lib.load().pram_mapbuild_vrf_workspace_bytes(n_lm, max(total, 0), F)), workspace, dev, floor=8)
    lm_vrf, lm_vrf_n = _new(dev, torch.int32, n_lm, max(n_vrf, 1)), _new(dev, torch.int32, n_lm)
    _call("pram_mapbuild_select_frames", s["point3D_ids"], s["frame_off"], F, int(s["n_rows"]), s["pt_ids"], s["pt_off"], s["pt_frames"], n_points,
          int(s["n_pt_entries"]), pt_xyz, lm_off, ctypes.addressof(host), lm_points, n_lm, frame_ignored, frame_cams, int(min_obs), int(topk_imgs), n_vrf,
          float(min_cover_ratio), float(gain_floor), workspace, workspace.numel(), lm_vrf, lm_vrf_n)
    return lm_vrf[:n_lm], lm_vrf_n[:n_lm]


# ---- map compression (csrc/compress.hip; pram_amd/localization/compress.py drives these) --------------------------------------
COMPRESS_ROW_TILE, COMPRESS_KPT_TILE = 256, 256      # include/pram_hip.h


def compress_workspace(store, device) -> torch.Tensor:
    return _ws(int(_lib.load().pram_compress_workspace_bytes(int(store["n_rows"]), int(store["covisibility_frame"]))), None, device, floor=8)


def compress_select(store, frame_off_host, covis_off_host, covis_frames_host, vrf_host, pt_xyz: torch.Tensor, xys: torch.Tensor,
                    frame_cams: torch.Tensor, radius: float, workspace: Optional[torch.Tensor] = None):
    """``store``: the device tables of a ReferenceStore (rows and point ids); the host copies of frame_off and of the covisibility
    graph, and the reference frames in order, as int arrays; pt_xyz float64 [n_points, 3]; xys float64 [n_rows, 2]; frame_cams
    float64 [F, MAPBUILD_CAM_COLS] -> (ret_order int32 [F]: place in the retained order or -1, list_cnt int32 [F], list_pt int32
    [n_rows]: frame f's kept rows as point table indices at frame_off[f] ..).  Nothing is read back."""
    s = store
    F, n_rows, n_points, cov = int(s["n_frames"]), int(s["n_rows"]), int(s["n_points"]), int(s["covisibility_frame"])
    _check((pt_xyz, "pt_xyz", torch.float64), (xys, "xys", torch.float64), (frame_cams, "frame_cams", torch.float64))
    fo, n_fo = _int_table(frame_off_host)
    co, n_co = _int_table(covis_off_host)
    cf, n_cf = _int_table(covis_frames_host)
    vh, n_vrf = _int_table(vrf_host)
    if n_fo != F + 1 or n_co != F + 1 or n_cf < int(co[F]) or F < 1:
        raise _lib.PramHipError(f"compress_select: frame_off and covis_off need {F + 1} entries (at least one frame), covis_frames {int(co[F]) if n_co == F + 1 else '?'}")
    assert pt_xyz.numel() >= 3 * n_points and xys.numel() >= 2 * n_rows and frame_cams.numel() >= F * MAPBUILD_CAM_COLS
    dev = pt_xyz.device
    if workspace is None:
        workspace = compress_workspace(s, dev)
    _chk(workspace, "workspace", torch.uint8)
    ret_order = torch.empty(F, device=dev, dtype=torch.int32)
    list_cnt = torch.empty(F, device=dev, dtype=torch.int32)
    list_pt = _new(dev, torch.int32, n_rows)
    _call("pram_compress_select", s["point3D_ids"], s["frame_off"], ctypes.addressof(fo), F, n_rows, s["pt_ids"], n_points, pt_xyz, xys, frame_cams,
          ctypes.addressof(co), ctypes.addressof(cf), cov, ctypes.addressof(vh), n_vrf, float(radius), workspace, workspace.numel(), ret_order, list_cnt,
          list_pt)
    return ret_order, list_cnt, list_pt


def compress_sparsify(store, frame_cams: torch.Tensor, pt_xyz: torch.Tensor, pt_score: torch.Tensor, radius: float, nkpts: int,
                      list_pt: torch.Tensor, list_cnt: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> None:
    """In place on (list_pt, list_cnt) of :func:`compress_select`: every frame listing more than ``nkpts`` points keeps the best
    point (pt_score int32 [n_points], the earlier on a tie) of every cell of ``radius`` pixels, in the order the cells appear."""
    s = store
    F, n_rows, n_points = int(s["n_frames"]), int(s["n_rows"]), int(s["n_points"])
    _check((frame_cams, "frame_cams", torch.float64, F * MAPBUILD_CAM_COLS), (pt_xyz, "pt_xyz", torch.float64, 3 * n_points),
           (pt_score, "pt_score", torch.int32, n_points), (list_pt, "list_pt", torch.int32, n_rows), (list_cnt, "list_cnt", torch.int32, F))
    if workspace is None:
        workspace = compress_workspace(s, pt_xyz.device)
    _chk(workspace, "workspace", torch.uint8)
    _call("pram_compress_sparsify", s["frame_off"], F, n_rows, frame_cams, pt_xyz, pt_score, n_points, float(radius), int(nkpts), workspace,
          workspace.numel(), list_pt, list_cnt)


def compress_rows(row_frame: torch.Tensor, row_point: torch.Tensor, n_frames: int, frame_cams: torch.Tensor, pt_ids: torch.Tensor,
                  pt_xyz: torch.Tensor, pt_desc: torch.Tensor, pt_sid: torch.Tensor, pt_err: torch.Tensor, n_points: int) -> dict:
    """Row i of a compressed map: point row_point[i] (index into the point table) seen from frame row_frame[i] -> dict(keypoints
    float64 [n, 3] (u, v, score), xyzs float64 [n, 3], descriptors float32 [n, 128], keypoint_segs int32 [n], point3D_ids int64 [n])."""
    n = int(row_frame.numel())
    _check((row_frame, "row_frame", torch.int32), (row_point, "row_point", torch.int32),
           (frame_cams, "frame_cams", torch.float64, int(n_frames) * MAPBUILD_CAM_COLS), (pt_ids, "pt_ids", _INT64, n_points),
           (pt_xyz, "pt_xyz", torch.float64, 3 * n_points), (pt_desc, "pt_desc", torch.float32, 128 * n_points),
           (pt_sid, "pt_sid", torch.int32, n_points), (pt_err, "pt_err", torch.float64, n_points))
    assert row_point.numel() == n
    dev = row_frame.device
    out = {"keypoints": _new(dev, torch.float64, n, 3), "xyzs": _new(dev, torch.float64, n, 3), "descriptors": _new(dev, torch.float32, n, 128),
           "keypoint_segs": _new(dev, torch.int32, n), "point3D_ids": _new(dev, _INT64, n)}
    _call("pram_compress_rows", row_frame, row_point, n, int(n_frames), int(n_points), frame_cams, pt_ids, pt_xyz, pt_desc, pt_sid, pt_err,
          out["keypoints"], out["xyzs"], out["descriptors"], out["keypoint_segs"], out["point3D_ids"])
    return {k: v[:n] for k, v in out.items()}


# ---- k-means labelling (csrc/kmeans.hip; pram_amd/localization/labelling.py drives these) --------------------------------------
KMEANS_BLOCK, KMEANS_MAX_K, KMEANS_MAX_TRIALS, KMEANS_STATE_WORDS = 1024, 4096, 10, 8      # include/pram_hip.h
KMEANS_DONE, KMEANS_ITER, KMEANS_STRICT, KMEANS_RELOC = 0, 1, 2, 3      # words of the state


def _kmeans_x(x: torch.Tensor, name: str = "x") -> int:
    _chk(x, name, torch.float64)
    if x.dim() != 2 or x.shape[1] != 3 or not x.is_contiguous():
        raise _lib.PramHipError(f"{name}: expected a contiguous float64 [n, 3] tensor, got {tuple(x.shape)}")
    return int(x.shape[0])


def kmeans_workspace(n: int, k: int, device) -> torch.Tensor:
    return _ws(int(_lib.load().pram_kmeans_workspace_bytes(int(n), int(k))), None, device,
               f"kmeans: needs 1 <= n < 2^31 and 1 <= k <= min(n, {KMEANS_MAX_K}), got n = {n}, k = {k}")


def kmeans_init_pp(x: torch.Tensor, k: int, first: int, rand: torch.Tensor, workspace: Optional[torch.Tensor] = None):
    """sklearn's k-means++ on the centred points x float64 [n, 3] with the host's random numbers: ``first`` the first seed, rand
    float64 [k - 1, T] the uniform numbers of every step -> (seeds int32 [k]: the chosen points, centers float64 [k, 3])."""
    n, k = _kmeans_x(x), int(k)
    _chk(rand, "rand", torch.float64)
    T = int(rand.shape[1]) if rand.dim() == 2 else 0
    if rand.dim() != 2 or not rand.is_contiguous() or rand.shape[0] < k - 1 or T < 1:
        raise _lib.PramHipError(f"rand: expected a contiguous float64 [k - 1, T] tensor with T >= 1, got {tuple(rand.shape)}")
    if workspace is None:
        workspace = kmeans_workspace(n, k, x.device)
    _chk(workspace, "workspace", torch.uint8)
    seeds, centers = _new(x.device, torch.int32, k), _new(x.device, torch.float64, k, 3)
    _call("pram_kmeans_init_pp", x, n, k, int(first), rand, T, workspace, workspace.numel(), seeds, centers)
    return seeds, centers


def kmeans_buffers(n: int, device) -> dict:
    """The outputs and the state of :func:`kmeans_lloyd`, which carries them from one group of iterations to the next."""
    return {"labels": torch.empty(n, device=device, dtype=torch.int32), "dist": torch.empty(n, device=device, dtype=torch.float64),
            "state": torch.zeros(KMEANS_STATE_WORDS, device=device, dtype=torch.int32), "inertia": torch.zeros(2, device=device, dtype=torch.float64)}


def kmeans_lloyd(x: torch.Tensor, centers: torch.Tensor, tol_abs: float, max_iter: int, first_iter: int, n_iters: int, finish: bool,
                 buffers: dict, workspace: torch.Tensor) -> None:
    """Enqueues Lloyd iterations first_iter .. first_iter + n_iters - 1 on ``centers`` float64 [k, 3] (in place) and, with
    ``finish``, the final labels, distances and inertia into ``buffers`` (:func:`kmeans_buffers`).  buffers["state"] says when the
    iterations are done (word KMEANS_DONE); later iterations then return at once.  Nothing is read back here."""
    n = _kmeans_x(x)
    k = _kmeans_x(centers, "centers")
    _chk(workspace, "workspace", torch.uint8)
    b = buffers
    _check((b["labels"], "labels", torch.int32, n), (b["dist"], "dist", torch.float64, n), (b["state"], "state", torch.int32, KMEANS_STATE_WORDS),
           (b["inertia"], "inertia", torch.float64, 2))
    _call("pram_kmeans_lloyd", x, n, k, centers, float(tol_abs), int(max_iter), int(first_iter), int(n_iters), int(bool(finish)), workspace,
          workspace.numel(), b["labels"], b["dist"], b["state"], b["inertia"])


def kmeans_assign(x: torch.Tensor, centers: torch.Tensor):
    """One assignment step: x float64 [n, 3], centers float64 [k, 3] (k <= n) -> (labels int32 [n], squared distance float64 [n]);
    the lowest centre index wins a tie."""
    n = _kmeans_x(x)
    k = _kmeans_x(centers, "centers")
    labels, dist = _new(x.device, torch.int32, n), _new(x.device, torch.float64, n)
    _call("pram_kmeans_assign", x, n, centers, k, labels, dist)
    return labels[:n], dist[:n]


# ---- triangulation (csrc/triangulate.hip; pram_amd/localization/triangulation.py drives these) --------------------------------
TRI_GN_STEPS, TRI_FRAME_COLS, TRI_CC_STATE_WORDS = 5, 16, 4      # include/pram_hip.h
TRI_CC_DONE = 1      # the word of the components' state that says the labels are final
TRI_ROW_FREE, TRI_ROW_TAKEN, TRI_ROW_DEAD = 0, 1, 2      # include/pram_hip.h


def _tri_views(norm, keypoints, table, cam_model, cam_params, n_frames: int, n_rows: int):
    """The five tensors stage 2b and stage 4 read of the frame table, and their sizes."""
    _check((norm, "norm", torch.float64, 2 * n_rows), (keypoints, "keypoints", torch.float32, 2 * n_rows),
           (table, "table", torch.float64, TRI_FRAME_COLS * n_frames), (cam_model, "cam_model", torch.int32, n_frames),
           (cam_params, "cam_params", torch.float64, POSE_CAM_PARAMS * n_frames))


def tri_frames(qvec: torch.Tensor, tvec: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor, cam_model_host) -> torch.Tensor:
    """cam_from_world poses qvec float64 [F, 4] (w, x, y, z), tvec float64 [F, 3] and the frames' cameras (cam_model int32 [F],
    cam_params float64 [F, POSE_CAM_PARAMS], cam_model_host: the ids on the host) -> the frame table float64 [F, TRI_FRAME_COLS]
    that tri_verify and tri_triangulate read.  Every tensor holds one row at least (the rows beyond F are not read)."""
    host, F = _int_table(cam_model_host)
    _check((qvec, "qvec", torch.float64, 4 * F), (tvec, "tvec", torch.float64, 3 * F), (cam_model, "cam_model", torch.int32, F),
           (cam_params, "cam_params", torch.float64, POSE_CAM_PARAMS * F))
    table = _new(qvec.device, torch.float64, F, TRI_FRAME_COLS)
    _call("pram_tri_frames", qvec, tvec, cam_model, cam_params, ctypes.addressof(host), F, table)
    return table


def tri_normalize(keypoints: torch.Tensor, frame_off: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor, cam_model_host,
                  n_rows: int, pixel_offset: float) -> torch.Tensor:
    """keypoints float32 [n_rows, 2] of all frames, frame_off int32 [F + 1] -> float64 [n_rows, 2] on the normalised plane of each
    row's frame, (x + pixel_offset, y + pixel_offset) undistorted as pose_prepare does."""
    (host, F), n_rows = _int_table(cam_model_host), int(n_rows)
    _check((keypoints, "keypoints", torch.float32, 2 * n_rows), (frame_off, "frame_off", torch.int32, F + 1), (cam_model, "cam_model", torch.int32, F),
           (cam_params, "cam_params", torch.float64, POSE_CAM_PARAMS * F))
    norm = _new(keypoints.device, torch.float64, n_rows, 2)
    _call("pram_tri_normalize", keypoints, frame_off, cam_model, cam_params, ctypes.addressof(host), F, n_rows, float(pixel_offset), norm)
    return norm


def tri_verify(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, matches: torch.Tensor,
               table: torch.Tensor, n_frames: int, n_pairs: int, n_matches: int, max_error: float) -> dict:
    """norm: tri_normalize with offset 0; pairs int32 [Pn, 2] frame indices; the matches as CSR, match_off int32 [Pn + 1] and
    matches int32 [M, 2] -> keep uint8 [M], kept int32 [M, 2] (pair p's kept matches from match_off[p] on, original order), edges
    int32 [M, 2] (rows, -1 where dropped), count int32 [Pn]."""
    F, Pn, M = int(n_frames), int(n_pairs), int(n_matches)
    _check((norm, "norm", torch.float64), (frame_off, "frame_off", torch.int32, F + 1), (pairs, "pairs", torch.int32, 2 * Pn),
           (match_off, "match_off", torch.int32, Pn + 1), (matches, "matches", torch.int32, 2 * M), (table, "table", torch.float64, TRI_FRAME_COLS * F))
    dev = norm.device
    out = {"keep": _new(dev, torch.uint8, M), "kept": _new(dev, torch.int32, M, 2), "edges": _new(dev, torch.int32, M, 2),
           "count": _new(dev, torch.int32, Pn)}
    _call("pram_tri_verify", norm, frame_off, pairs, match_off, matches, table, F, Pn, M, float(max_error), out["keep"], out["kept"], out["edges"],
          out["count"])
    return out


def tri_components(edges: torch.Tensor, n_edges: int, n_rows: int, first_round: int, n_rounds: int, label: torch.Tensor, state: torch.Tensor):
    """Rounds first_round .. first_round + n_rounds - 1 of the connected components over rows (edges int32 [n_edges, 2]) on label
    int32 [n_rows] and state int32 [TRI_CC_STATE_WORDS]; state[TRI_CC_DONE] says when label holds every row's smallest row."""
    _check((edges, "edges", torch.int32, 2 * int(n_edges)), (label, "label", torch.int32, int(n_rows)), (state, "state", torch.int32, TRI_CC_STATE_WORDS))
    _call("pram_tri_components", edges, int(n_edges), int(n_rows), int(first_round), int(n_rounds), label, state)


def tri_tracks(label: torch.Tensor, frame_off: torch.Tensor, n_frames: int, n_rows: int, workspace: Optional[torch.Tensor] = None) -> dict:
    """label int32 [n_rows] (tri_components) -> the tracks as CSR, sized for the worst case: trk_off int32 [n_rows // 2 + 2],
    trk_label int32 [n_rows // 2 + 1], trk_row / trk_frame / trk_kpt int32 [n_rows], and sizes int32 [2] = (tracks, entries), all on
    the device.  ``workspace``: uint8, at least pram_tri_tracks_workspace_bytes; None allocates it."""
    F, n = int(n_frames), int(n_rows)
    _check((label, "label", torch.int32, n), (frame_off, "frame_off", torch.int32, F + 1))
    dev = label.device
    workspace = _ws(int(_lib.load().pram_tri_tracks_workspace_bytes(n)), workspace, dev, "pram_tri_tracks: more than 2^30 rows")
    out = {"trk_off": _new(dev, torch.int32, n // 2 + 2), "trk_label": _new(dev, torch.int32, n // 2 + 1), "trk_row": _new(dev, torch.int32, n),
           "trk_frame": _new(dev, torch.int32, n), "trk_kpt": _new(dev, torch.int32, n), "sizes": _new(dev, torch.int32, 2)}
    _call("pram_tri_tracks", label, frame_off, F, n, workspace, workspace.numel(), out["trk_off"], out["trk_label"], out["trk_row"], out["trk_frame"],
          out["trk_kpt"], out["sizes"])
    return out


def tri_triangulate(norm: torch.Tensor, keypoints: torch.Tensor, table: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor,
                    trk_off: torch.Tensor, trk_label: torch.Tensor, trk_row: torch.Tensor, trk_frame: torch.Tensor, n_tracks: int,
                    n_entries: int, n_frames: int, n_rows: int, trials: int = 128, seed: int = 0, min_tri_angle: float = 0.026179938779914945,
                    max_reproj_error: float = 4.0) -> dict:
    """norm: tri_normalize with offset 0.5; the tracks of tri_tracks (or a caller's own table) -> accept int32 [T], xyz float64
    [T, 3], error float64 [T], kept int32 [T], best int32 [T] (the winning hypothesis, -1: none), entry_keep uint8 [E], entry_error
    float64 [E].  min_tri_angle in radians."""
    T, E, F, n = int(n_tracks), int(n_entries), int(n_frames), int(n_rows)
    _tri_views(norm, keypoints, table, cam_model, cam_params, F, n)
    _check((trk_off, "trk_off", torch.int32, T + 1), (trk_label, "trk_label", torch.int32, T), (trk_row, "trk_row", torch.int32, E),
           (trk_frame, "trk_frame", torch.int32, E))
    dev = norm.device
    out = {"accept": _new(dev, torch.int32, T), "xyz": _new(dev, torch.float64, T, 3), "error": _new(dev, torch.float64, T),
           "kept": _new(dev, torch.int32, T), "best": _new(dev, torch.int32, T), "entry_keep": _new(dev, torch.uint8, E),
           "entry_error": _new(dev, torch.float64, E)}
    _call("pram_tri_triangulate", norm, keypoints, table, cam_model, cam_params, trk_off, trk_label, trk_row, trk_frame, T, E, F, n, int(trials),
          int(seed) & 0xFFFFFFFFFFFFFFFF, float(min_tri_angle), float(max_reproj_error), out["accept"], out["xyz"], out["error"], out["kept"],
          out["best"], out["entry_keep"], out["entry_error"])
    return out


def tri_adjacency(edges: torch.Tensor, n_edges: int, frame_off: torch.Tensor, n_frames: int, n_rows: int,
                  workspace: Optional[torch.Tensor] = None) -> dict:
    """edges int32 [n_edges, 2] rows (an edge with an end outside [0, n_rows) or with equal ends is skipped) -> the rows' adjacency
    on the device: adj_off int32 [n_rows + 1], adj int32 [2 * n_edges] (adj_off[n_rows] of them written, every row's list
    ascending, duplicates kept) and row_frame int32 [n_rows].  ``workspace``: uint8, at least
    pram_tri_adjacency_workspace_bytes; None allocates it."""
    m, F, n = int(n_edges), int(n_frames), int(n_rows)
    _check((edges, "edges", torch.int32, 2 * m), (frame_off, "frame_off", torch.int32, F + 1))
    dev = edges.device
    workspace = _ws(int(_lib.load().pram_tri_adjacency_workspace_bytes(n, m)), workspace, dev,
                    "pram_tri_adjacency: more than 2^30 rows or 2^30 - 1 edges")
    out = {"adj_off": _new(dev, torch.int32, n + 1), "adj": _new(dev, torch.int32, 2 * m), "row_frame": _new(dev, torch.int32, n)}
    _call("pram_tri_adjacency", edges, m, frame_off, F, n, workspace, workspace.numel(), out["adj_off"], out["adj"], out["row_frame"])
    return out


def tri_support(norm: torch.Tensor, keypoints: torch.Tensor, table: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor,
                edges: torch.Tensor, n_edges: int, adj_off: torch.Tensor, adj: torch.Tensor, row_frame: torch.Tensor, n_frames: int,
                n_rows: int, min_tri_angle: float = 0.026179938779914945, max_reproj_error: float = 4.0, min_support: int = 1) -> dict:
    """norm: tri_normalize with offset 0.5; adj_off / adj / row_frame: tri_adjacency over the same edges -> support int32 [n_edges]
    (the witnesses of third frames that confirm the edge) and edges int32 [n_edges, 2]: the edge where support >= min_support,
    (-1, -1) elsewhere.  min_tri_angle in radians."""
    m, F, n = int(n_edges), int(n_frames), int(n_rows)
    _tri_views(norm, keypoints, table, cam_model, cam_params, F, n)
    _check((edges, "edges", torch.int32, 2 * m), (adj_off, "adj_off", torch.int32, n + 1), (adj, "adj", torch.int32, 2 * m),
           (row_frame, "row_frame", torch.int32, n))
    dev = norm.device
    out = {"support": _new(dev, torch.int32, m), "edges": _new(dev, torch.int32, m, 2)}
    _call("pram_tri_support", norm, keypoints, table, cam_model, cam_params, edges, m, adj_off, adj, row_frame, F, n, float(min_tri_angle),
          float(max_reproj_error), int(min_support), out["support"], out["edges"])
    return out


def tri_split(trk_off: torch.Tensor, trk_row: torch.Tensor, n_tracks: int, n_entries: int, accept: torch.Tensor, entry_keep: torch.Tensor,
              edges: torch.Tensor, n_edges: int, n_rows: int, state: Optional[torch.Tensor] = None) -> dict:
    """One round's track table (tri_tracks) and results (tri_triangulate's accept and entry_keep) and the edges the first round's
    tracks came from -> state uint8 [n_rows] (TRI_ROW_*; ``state`` updated in place, None: a new one that starts all DEAD), edges
    int32 [n_edges, 2]: the edge where both ends are FREE, (-1, -1) elsewhere, and n_live int32 [1], the number of such edges, on
    the device."""
    T, E, m, n = int(n_tracks), int(n_entries), int(n_edges), int(n_rows)
    _check((trk_off, "trk_off", torch.int32, T + 1), (trk_row, "trk_row", torch.int32, E), (accept, "accept", torch.int32, T),
           (entry_keep, "entry_keep", torch.uint8, E), (edges, "edges", torch.int32, 2 * m))
    dev = edges.device
    first = state is None
    if first:
        state = _new(dev, torch.uint8, n)
    _check((state, "state", torch.uint8, n))
    out = {"state": state, "edges": _new(dev, torch.int32, m, 2), "n_live": _new(dev, torch.int32, 1)}
    _call("pram_tri_split", trk_off, trk_row, T, E, accept, entry_keep, edges, m, n, int(first), state, out["edges"], out["n_live"])
    return out


# ---- two-view geometry without poses (csrc/twoview.hip; pram_amd/localization/twoview.py drives these) ------------------------
TWOVIEW_MAX_SOL = 10      # PRAM_TWOVIEW_MAX_SOL
TWOVIEW_TRIAL_BYTES = TWOVIEW_MAX_SOL * (9 * 8 + 4 + 8) + 4      # hypotheses, counts, residual sums and n_sol of one trial


def _twoview_views(norm, frame_off, pairs, match_off, matches, n_frames: int, n_pairs: int, n_matches: int):
    """The five tensors every two-view entry reads of the frame table and the match CSR, and their sizes."""
    _check((norm, "norm", torch.float64), (frame_off, "frame_off", torch.int32, n_frames + 1), (pairs, "pairs", torch.int32, 2 * n_pairs),
           (match_off, "match_off", torch.int32, n_pairs + 1), (matches, "matches", torch.int32, 2 * n_matches))


def _twoview_cams(cam_model, cam_params, n_frames: int):
    _check((cam_model, "cam_model", torch.int32, n_frames), (cam_params, "cam_params", torch.float64, POSE_CAM_PARAMS * n_frames))


def twoview_hypotheses(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, matches: torch.Tensor,
                       n_frames: int, n_pairs: int, n_matches: int, first_pair: int = 0, trials: int = 1024, seed: int = 0,
                       return_fives: bool = False) -> dict:
    """norm: tri_normalize with offset 0.5; pairs int32 [Pn, 2]; the matches as CSR (match_off int32 [Pn + 1], matches int32 [M, 2])
    -> E float64 [Pn, trials, TWOVIEW_MAX_SOL, 9] (the kept roots of every five-point sample first, zeros behind), n_sol int32
    [Pn, trials] and, with return_fives, fives int32 [Pn, trials, 5].  first_pair: the position of pairs[0] among all processed
    pairs (the sampler's key)."""
    F, Pn, M, T = int(n_frames), int(n_pairs), int(n_matches), int(trials)
    _twoview_views(norm, frame_off, pairs, match_off, matches, F, Pn, M)
    dev = norm.device
    out = {"E": _new(dev, torch.float64, Pn, T, TWOVIEW_MAX_SOL, 9), "n_sol": _new(dev, torch.int32, Pn, T)}
    if return_fives:
        out["fives"] = _new(dev, torch.int32, Pn, T, 5)
    _call("pram_twoview_hypotheses", norm, frame_off, pairs, match_off, matches, F, Pn, M, int(first_pair), T, int(seed) & 0xFFFFFFFFFFFFFFFF,
          out["E"], out["n_sol"], out.get("fives"))
    return out


def twoview_score(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, matches: torch.Tensor,
                  cam_model: torch.Tensor, cam_params: torch.Tensor, n_frames: int, n_pairs: int, n_matches: int, E: torch.Tensor,
                  n_sol: torch.Tensor, max_error: float = 4.0) -> dict:
    """E float64 [Pn, trials, TWOVIEW_MAX_SOL, 9] and n_sol int32 [Pn, trials] (twoview_hypotheses') -> h_inliers int32
    [Pn, trials, TWOVIEW_MAX_SOL] (-1 for an empty slot), h_resid float64 (same shape), best int32 [Pn] (-1: no slot)."""
    F, Pn, M = int(n_frames), int(n_pairs), int(n_matches)
    _twoview_views(norm, frame_off, pairs, match_off, matches, F, Pn, M)
    _twoview_cams(cam_model, cam_params, F)
    _check((E, "E", torch.float64), (n_sol, "n_sol", torch.int32))
    assert E.dim() == 4 and tuple(E.shape[2:]) == (TWOVIEW_MAX_SOL, 9) and E.shape[0] >= Pn and tuple(n_sol.shape) == tuple(E.shape[:2])
    T, dev = int(E.shape[1]), norm.device
    out = {"h_inliers": _new(dev, torch.int32, Pn, T, TWOVIEW_MAX_SOL), "h_resid": _new(dev, torch.float64, Pn, T, TWOVIEW_MAX_SOL),
           "best": _new(dev, torch.int32, Pn)}
    _call("pram_twoview_score", norm, frame_off, pairs, match_off, matches, cam_model, cam_params, F, Pn, M, E, n_sol, T, float(max_error),
          out["h_inliers"], out["h_resid"], out["best"])
    return out


_TWOVIEW_PAIR_OUT = (("E", torch.float64, (9,)), ("qvec", torch.float64, (4,)), ("tvec", torch.float64, (3,)), ("num_inliers", torch.int32, ()),
                     ("num_front", torch.int32, ()), ("success", torch.int32, ()), ("count", torch.int32, ()))
_TWOVIEW_MATCH_OUT = (("keep", torch.uint8, ()), ("kept", torch.int32, (2,)), ("edges", torch.int32, (2,)))


def twoview_outputs(n_pairs: int, n_matches: int, device) -> dict:
    """What twoview_finish writes, allocated: E float64 [Pn, 9], qvec [Pn, 4], tvec [Pn, 3], num_inliers / num_front / success /
    count int32 [Pn], and tri_verify's keep uint8 [M], kept int32 [M, 2], edges int32 [M, 2]."""
    out = {k: _new(device, dt, int(n_pairs), *sh) for k, dt, sh in _TWOVIEW_PAIR_OUT}
    out.update({k: _new(device, dt, int(n_matches), *sh) for k, dt, sh in _TWOVIEW_MATCH_OUT})
    return out


def twoview_finish(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, matches: torch.Tensor,
                   cam_model: torch.Tensor, cam_params: torch.Tensor, n_frames: int, n_pairs: int, n_matches: int, E: torch.Tensor,
                   h_inliers: torch.Tensor, best: torch.Tensor, max_error: float = 4.0, min_inlier_ratio: float = 0.1,
                   min_num_inliers: int = 15, refine_iters: int = 20, out: Optional[dict] = None) -> dict:
    """The best slot of every pair (twoview_score's) decomposed, refined and scored again -> twoview_outputs' dict.  ``out``: that
    dict with the per-pair tensors cut to this call's pairs and the per-match tensors whole (match_off indexes them), so that a
    caller walks a long pair list in chunks; None allocates it."""
    F, Pn, M = int(n_frames), int(n_pairs), int(n_matches)
    _twoview_views(norm, frame_off, pairs, match_off, matches, F, Pn, M)
    _twoview_cams(cam_model, cam_params, F)
    _check((E, "E", torch.float64), (h_inliers, "h_inliers", torch.int32), (best, "best", torch.int32, Pn))
    assert E.dim() == 4 and tuple(E.shape[2:]) == (TWOVIEW_MAX_SOL, 9) and E.shape[0] >= Pn and tuple(h_inliers.shape) == tuple(E.shape[:3])
    if out is None:
        out = twoview_outputs(Pn, M, norm.device)
    _check(*[(out[k], k, dt, Pn * (sh[0] if sh else 1)) for k, dt, sh in _TWOVIEW_PAIR_OUT],
           *[(out[k], k, dt, M * (sh[0] if sh else 1)) for k, dt, sh in _TWOVIEW_MATCH_OUT])
    _call("pram_twoview_finish", norm, frame_off, pairs, match_off, matches, cam_model, cam_params, F, Pn, M, E, h_inliers, best, int(E.shape[1]),
          float(max_error), float(min_inlier_ratio), int(min_num_inliers), int(refine_iters), out["E"], out["qvec"], out["tvec"], out["num_inliers"],
          out["num_front"], out["success"], out["keep"], out["kept"], out["edges"], out["count"])
    return out


# ---- statistical outlier removal (csrc/knn.hip; pram_amd/localization/outliers.py drives these) -------------------------------
KNN_TILE, KNN_MAX_K, SOR_BLOCK = 1024, 32, 1024      # include/pram_hip.h
SOR_MEAN, SOR_STD, SOR_THRESHOLD, SOR_NV = 0, 1, 2, 3      # entries of the statistics


def knn_mean_distance(x: torch.Tensor, k: int) -> torch.Tensor:
    """x float64 [n, 3] -> float64 [n]: every point's mean distance to its min(k, n) nearest points, itself included (all pairs,
    exact).  1 <= k <= KNN_MAX_K."""
    n = _kmeans_x(x)
    avg = _new(x.device, torch.float64, n)
    _call("pram_knn_mean_distance", x, n, int(k), avg)
    return avg[:n]


def sor_workspace(n: int, device) -> torch.Tensor:
    return _ws(int(_lib.load().pram_sor_workspace_bytes(int(n))), None, device, f"sor_select: needs 1 <= n < 2^31, got n = {n}")


def sor_select(avg: torch.Tensor, std_ratio: float, workspace: Optional[torch.Tensor] = None) -> dict:
    """avg float64 [n] (:func:`knn_mean_distance`) -> stats float64 [4] (mean, std, threshold and the number of valid points, over
    the points with avg > 0), mask uint8 [n] (valid and avg < threshold), inlier_idx int32 [n] (the inliers' indices, ascending;
    the entries beyond count[0] are unspecified) and count int32 [2] (inliers, valid points).  Nothing is read back."""
    _chk(avg, "avg", torch.float64)
    if avg.dim() != 1 or not avg.is_contiguous():
        raise _lib.PramHipError(f"avg: expected a contiguous float64 [n] tensor, got {tuple(avg.shape)}")
    n, dev = int(avg.shape[0]), avg.device
    if workspace is None:
        workspace = sor_workspace(n, dev)
    _chk(workspace, "workspace", torch.uint8)
    out = {"stats": _new(dev, torch.float64, 4), "mask": _new(dev, torch.uint8, n), "inlier_idx": _new(dev, torch.int32, n),
           "count": _new(dev, torch.int32, 2)}
    _call("pram_sor_select", avg, n, float(std_ratio), workspace, workspace.numel(), out["stats"], out["mask"], out["inlier_idx"], out["count"])
    out["mask"], out["inlier_idx"] = out["mask"][:n], out["inlier_idx"][:n]
    return out


# ---- localisation against retrieved database frames (csrc/retrieval.hip; pram_amd/localization/retrieval.py drives these) ----
COVIS_WORKSPACE_BYTES = 64 << 20      # the histogram [n, n_frames] of one covis_topk call stays under this: longer lists go in chunks


def retr_plan(retrieval: torch.Tensor, counts: torch.Tensor, store, enable: Optional[torch.Tensor] = None) -> torch.Tensor:
    """retrieval int32 [B, n_db] (store frame indices, -1 padded), counts int32 [B], ``store``: the device tables of a DatabaseStore
    -> plan int32 [CAND_PLAN_COLS, B * n_db] whose sel_off points into valid_rows."""
    _check((retrieval, "retrieval", torch.int32), (counts, "counts", torch.int32), *(((enable, "enable", torch.int32),) if enable is not None else ()))
    assert retrieval.dim() == 2 and counts.numel() == retrieval.shape[0] and (enable is None or enable.numel() == counts.numel())
    B, n_db = retrieval.shape
    plan = torch.empty(CAND_PLAN_COLS, B * n_db, device=retrieval.device, dtype=torch.int32)
    s = store
    _call("pram_retr_plan", retrieval, counts, enable, s["frame_off"], s["valid_off"], B, n_db, int(s["n_frames"]), int(s["n_valid"]), plan)
    return plan


def retr_filter(cor: dict, store, obs_th: int, out: Optional[dict] = None) -> dict:
    """cor: cand_correspond's dict -> the same lists [P, t0, ...] holding, per pair and in order, the rows whose point has obs_th
    observations or more, and their count.  ``out``: buffers to write into (the tests pre-fill them)."""
    P, t0 = _cor_chk(cor, "correspondences")
    if out is None:
        out = _cor_alloc(P, t0, cor["count"].device)
    else:
        assert _cor_chk(out, "out") == (P, t0)
    s = store
    _call("pram_retr_filter", *[cor[k] for k in MATCH_KEYS], cor["count"], P, t0, s["pt_ids"], s["pt_off"], int(s["n_points"]), int(obs_th),
          *[out[k] for k in MATCH_KEYS], out["count"])
    return out


def retr_select(success: torch.Tensor, num_inliers: torch.Tensor, count: torch.Tensor, n_db: int, inlier_th: int, min_best_inliers: int) -> torch.Tensor:
    """success / num_inliers / count int32 [B * n_db] -> int32 [B, 3]: kept slot (-1 none), status (1 accepted, 2 best taken, 0
    failed), best slot (-1 none)."""
    _check((success, "success", torch.int32), (num_inliers, "num_inliers", torch.int32), (count, "count", torch.int32))
    n_db = int(n_db)
    assert num_inliers.numel() == success.numel() and count.numel() == success.numel()
    assert n_db >= 1 and success.numel() % n_db == 0
    B = success.numel() // n_db
    chosen = torch.empty(B, 3, device=success.device, dtype=torch.int32)
    _call("pram_retr_select", success, num_inliers, count, B, n_db, int(inlier_th), int(min_best_inliers), chosen)
    return chosen


def covis_topk(frames: torch.Tensor, store, k: int, include_self: bool = False, workspace: Optional[torch.Tensor] = None):
    """frames int32 [n] (store frame indices), ``store``: the device tables of a DatabaseStore -> (best_frames int32 [n, k] (-1
    padded), best_counts int32 [n, k], n_found int32 [n]).  workspace: int32 [>= min(n, chunk) * n_frames], dirty or not; the
    frames go through the entry in chunks whose histogram stays under COVIS_WORKSPACE_BYTES."""
    _check((frames, "frames", torch.int32))
    assert frames.dim() == 1
    n, k, s, dev = frames.numel(), int(k), store, frames.device
    F = max(int(s["n_frames"]), 1)
    chunk = max(1, min(max(n, 1), COVIS_WORKSPACE_BYTES // (4 * F)))
    if workspace is None:
        workspace = torch.empty(chunk * F, device=dev, dtype=torch.int32)
    _check((workspace, "workspace", torch.int32, chunk * F))
    best_f, best_c = _new(dev, torch.int32, n, max(k, 1)), _new(dev, torch.int32, n, max(k, 1))
    n_found = _new(dev, torch.int32, n)
    for a in range(0, max(n, 1), chunk):
        _call("pram_covis_topk", frames[a:] if n else n_found, min(chunk, n - a), s["valid_off"], s["valid_rows"], s["point3D_ids"], int(s["n_rows"]),
              int(s["n_valid"]), s["pt_ids"], s["pt_off"], s["pt_frames"], int(s["n_points"]), int(s["n_pt_entries"]), int(s["n_frames"]), k,
              int(bool(include_self)), workspace, best_f[a:], best_c[a:], n_found[a:])
    return best_f[:n], best_c[:n], n_found[:n]


# ---- bundle adjustment (csrc/bundle.hip; pram_amd/localization/bundle.py drives these) ----------------------------------------
BA_OBS_DOUBLES, BA_BLOCK, BA_CONTEXT_BYTES, BA_STATE_F64, BA_STATE_I32 = 20, 64, 512, 16, 16      # include/pram_hip.h
BA_SD_COST, BA_SD_LAM, BA_SD_COST0 = 0, 2, 9      # words of the state's float64 part
BA_SI_DONE, BA_SI_REASON, BA_SI_LM_ITER, BA_SI_ACCEPTED, BA_SI_CG_FAIL = 0, 1, 2, 3, 9      # and of its int32 part
BA_REASONS = {0: "running", 1: "max_iters", 2: "ftol", 3: "tables"}      # PRAM_BA_REASON_*
BA_STAGE_LINEARISE, BA_STAGE_BLOCKS, BA_STAGE_CG_INIT, BA_STAGE_CG, BA_STAGE_STEP, BA_STAGE_ALL = 1, 2, 4, 8, 16, 31
# the workspace's arrays in bundle.hip's order: name, dtype, columns (0: the count comes with the sizes)
BA_ARRAYS = (("table", torch.float64, "F", 16), ("table_cand", torch.float64, "F", 16), ("xyz", torch.float64, "P", 3), ("xyz_cand", torch.float64, "P", 3),
             ("jac", torch.float64, "O", 20), ("v_inv", torch.float64, "P", 6), ("g_p", torch.float64, "P", 3), ("y_p", torch.float64, "P", 3),
             ("s_block", torch.float64, "F", 21), ("diag_u", torch.float64, "F", 6), ("b", torch.float64, "F", 6), ("cg_x", torch.float64, "F", 6),
             ("cg_r", torch.float64, "F", 6), ("cg_z", torch.float64, "F", 6), ("cg_p", torch.float64, "F", 6), ("cg_q", torch.float64, "F", 6),
             ("frame_dot", torch.float64, "F2", 1), ("frame_cost", torch.float64, "F", 1), ("partials", torch.float64, "B2", 1),
             ("state_f64", torch.float64, "SD", 1), ("state_i32", torch.int32, "SI", 1), ("point_ok", torch.int32, "P", 1),
             ("moved", torch.int32, "F", 1), ("frozen", torch.int32, "F", 1), ("obs_ok", torch.uint8, "O", 1))
_BA_OBS_NAMES = ("obs_row", "obs_frame", "obs_point", "frm_off", "pt_off", "pt_obs", "frozen")
_BA_GROUP_NAMES = ("frm_grp", "grp_off", "grp_frame", "grp_params", "grp_mask")


def _ba_begin(keypoints, cam_model, cam_params, cam_model_host, table, xyz, obs, n_points, n_obs, n_rows, max_iters, loss_scale, lam0, cg_tol, ftol,
              groups=None, n_groups=0) -> dict:
    """ba_begin (cam_params given, groups None) or bac_begin (cam_params None, groups = the tensors of _BA_GROUP_NAMES); obs = the
    tensors of _BA_OBS_NAMES."""
    cam = groups is not None
    host, F = _int_table(cam_model_host)
    Pn, O, n, G, K = int(n_points), int(n_obs), int(n_rows), int(n_groups), int(max_iters)
    if F < 1 or Pn < 1 or O < 1 or n < 1 or (cam and not 1 <= G <= F):
        raise _lib.PramHipError("bac_begin: needs one frame, one point, one observation and one keypoint at least, and 1 <= groups <= frames" if cam
                                else "ba_begin: needs one frame, one point, one observation and one keypoint at least")
    _check((keypoints, "keypoints", torch.float32, 2 * n), (table, "table", torch.float64, TRI_FRAME_COLS * F), (xyz, "xyz", torch.float64, 3 * Pn),
           (cam_model, "cam_model", torch.int32, F), *[(t, nm, torch.int32, least) for t, nm, least in zip(obs, _BA_OBS_NAMES, (O, O, O, F + 1, Pn + 1, O, F))])
    if cam:
        _check(*[(t, nm, torch.float64 if nm == "grp_params" else torch.int32, least)
                 for t, nm, least in zip(groups, _BA_GROUP_NAMES, (F, G + 1, F, BAC_GROUP_PARAMS * G, G))])
    else:
        _check((cam_params, "cam_params", torch.float64, POSE_CAM_PARAMS * F))
    L = _lib.load()
    entry, arrays, sizes = ("pram_bac", BAC_ARRAYS, (F, Pn, O, G, K)) if cam else ("pram_ba", BA_ARRAYS, (F, Pn, O, K))
    workspace = _ws(int(getattr(L, entry + "_workspace_bytes")(*sizes)), None, keypoints.device,
                    entry + "_begin: sizes beyond 2^24 frames, 2^28 points, 2^26 observations or 4096 iterations")
    offsets = (ctypes.c_size_t * (len(arrays) + 1))()
    _lib.check(getattr(L, entry + "_layout")(*sizes, ctypes.addressof(offsets)), entry + "_layout")
    count = {"F": F, "P": Pn, "O": O, "F2": 2 * F, "B2": 2 * ((F + BA_BLOCK - 1) // BA_BLOCK), "SD": BA_STATE_F64, "SI": BA_STATE_I32 + 2 * K,
             "G": G, "G2": 2 * G, "C2": 2 * ((G + BA_BLOCK - 1) // BA_BLOCK), "FB": F // BA_BLOCK + G + 1}
    views = {}
    for (name, dt, cnt, cols), a in zip(arrays, offsets):
        nbytes = count[cnt] * cols * torch.empty(0, dtype=dt).element_size()
        v = workspace[a:a + nbytes].view(dt)
        views[name] = v.view(count[cnt], cols) if cols > 1 else v
    context = ctypes.create_string_buffer(BAC_CONTEXT_BYTES if cam else BA_CONTEXT_BYTES)
    head = (keypoints, cam_model) + (() if cam else (cam_params,))      # the host's models follow these in both entries
    rest = (table, xyz) + tuple(obs) + (tuple(groups) if cam else ())
    _call(entry + "_begin", *head, ctypes.addressof(host), *rest, F, Pn, O, n, *((G,) if cam else ()), K, float(loss_scale), float(lam0),
          float(cg_tol), float(ftol), workspace, workspace.numel(), ctypes.addressof(context))
    problem = {"context": context, "workspace": workspace, "views": views, "n_frames": F, "n_points": Pn, "n_obs": O}
    problem.update({"n_groups": G, "max_iters": K, "cam": True} if cam else {"max_iters": K})
    problem["keep"] = head + rest
    return problem


def _ba_iterate(cam: bool, problem: dict, n_iters: int, cg_iters: int, stages: int):
    _call("pram_bac_iterate" if cam else "pram_ba_iterate", ctypes.addressof(problem["context"]), int(n_iters), int(cg_iters), int(stages))


def _ba_finish(cam: bool, problem: dict, qvec: torch.Tensor, tvec: torch.Tensor, max_reproj_error: float, min_tri_angle: float) -> dict:
    F, Pn, O = problem["n_frames"], problem["n_points"], problem["n_obs"]
    _check((qvec, "qvec", torch.float64, 4 * F), (tvec, "tvec", torch.float64, 3 * F))
    dev = qvec.device
    out = {"qvec": _new(dev, torch.float64, F, 4), "tvec": _new(dev, torch.float64, F, 3), "xyz": _new(dev, torch.float64, Pn, 3),
           "obs_keep": _new(dev, torch.uint8, O), "obs_error": _new(dev, torch.float64, O), "pt_keep": _new(dev, torch.int32, Pn),
           "pt_error": _new(dev, torch.float64, Pn), "pt_angle": _new(dev, torch.float64, Pn), "pt_kept": _new(dev, torch.int32, Pn),
           "counts": _new(dev, torch.int32, 2)}
    if cam:
        out["grp_params"] = _new(dev, torch.float64, problem["n_groups"], BAC_GROUP_PARAMS)
    _call("pram_bac_finish" if cam else "pram_ba_finish", ctypes.addressof(problem["context"]), qvec, tvec, float(max_reproj_error),
          float(min_tri_angle), out["qvec"], out["tvec"], out["xyz"], out["obs_keep"], out["obs_error"], out["pt_keep"], out["pt_error"],
          out["pt_angle"], out["pt_kept"], out["counts"], *((out["grp_params"],) if cam else ()))
    return out


def ba_begin(keypoints: torch.Tensor, cam_model: torch.Tensor, cam_params: torch.Tensor, cam_model_host, table: torch.Tensor, xyz: torch.Tensor,
             obs_row: torch.Tensor, obs_frame: torch.Tensor, obs_point: torch.Tensor, frm_off: torch.Tensor, pt_off: torch.Tensor,
             pt_obs: torch.Tensor, frozen: torch.Tensor, n_points: int, n_obs: int, n_rows: int, max_iters: int, loss_scale: float = 1.0,
             lam0: float = 1e-3, cg_tol: float = 1e-2, ftol: float = 1e-6) -> dict:
    """The problem of pram_ba_begin (include/pram_hip.h has the tables) -> a dict that holds the context, the workspace, the
    tensors the context points to (so that they outlive it) and ``views``: the workspace's arrays by BA_ARRAYS' names.  The initial
    cost is enqueued; nothing is read back."""
    return _ba_begin(keypoints, cam_model, cam_params, cam_model_host, table, xyz, (obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen),
                     n_points, n_obs, n_rows, max_iters, loss_scale, lam0, cg_tol, ftol)


def ba_iterate(problem: dict, n_iters: int, cg_iters: int, stages: int = BA_STAGE_ALL):
    """Enqueues n_iters Levenberg-Marquardt iterations of at most cg_iters conjugate-gradient iterations each on ``problem``
    (ba_begin's); ``stages``: BA_STAGE_* bits, for the tests and the timing tool.  Nothing is read back: the caller looks at
    problem["views"]["state_i32"][BA_SI_DONE] once per group of iterations."""
    _ba_iterate(False, problem, n_iters, cg_iters, stages)


def ba_finish(problem: dict, qvec: torch.Tensor, tvec: torch.Tensor, max_reproj_error: float = 4.0, min_tri_angle: float = 0.026179938779914945) -> dict:
    """qvec float64 [F, 4], tvec float64 [F, 3]: the poses the problem's table was made from -> the refined qvec / tvec (a frame
    that never moved keeps its input bit for bit), xyz float64 [P, 3], obs_keep uint8 [O], obs_error float64 [O], pt_keep int32 [P],
    pt_error / pt_angle float64 [P], pt_kept int32 [P] and counts int32 [2] (weight-0 observations at the final state, observations
    not kept).  min_tri_angle in radians."""
    return _ba_finish(False, problem, qvec, tvec, max_reproj_error, min_tri_angle)


# ---- bundle adjustment with camera groups (csrc/bundle.hip's pram_bac_*: DESIGN.md 4.27) ---------------------------------------
BAC_OBS_DOUBLES, BAC_GROUP_PARAMS, BAC_CONTEXT_BYTES = 36, 8, 1024      # include/pram_hip.h
CAMERA_NUM_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8}      # by PRAM_CAM_* id, COLMAP's counts
# the workspace's arrays: BA_ARRAYS with rows of BAC_OBS_DOUBLES, then the groups' (G: groups, G2: 2 G, C2: 2 ceil(G / BA_BLOCK), FB: F / BA_BLOCK + G + 1)
BAC_ARRAYS = tuple((n, dt, c, BAC_OBS_DOUBLES if n == "jac" else k) for n, dt, c, k in BA_ARRAYS) + (
    ("cam_params", torch.float64, "F", 8), ("cam_params_cand", torch.float64, "F", 8), ("grp_params", torch.float64, "G", 8),
    ("grp_params_cand", torch.float64, "G", 8), ("g_block", torch.float64, "G", 36), ("g_diag_u", torch.float64, "G", 8), ("g_b", torch.float64, "G", 8),
    ("g_cg_x", torch.float64, "G", 8), ("g_cg_r", torch.float64, "G", 8), ("g_cg_z", torch.float64, "G", 8), ("g_cg_p", torch.float64, "G", 8),
    ("g_cg_q", torch.float64, "G", 8), ("group_dot", torch.float64, "G2", 1), ("g_partials", torch.float64, "C2", 1),
    ("frame_group_sums", torch.float64, "F", 60), ("frame_mv_sums", torch.float64, "F", 8), ("grp_mask", torch.int32, "G", 1),
    ("grp_bad", torch.int32, "G", 1), ("grp_model", torch.int32, "G", 1), ("fold_blocks", torch.float64, "FB", 60))


def bac_begin(keypoints: torch.Tensor, cam_model: torch.Tensor, cam_model_host, table: torch.Tensor, xyz: torch.Tensor, obs_row: torch.Tensor,
              obs_frame: torch.Tensor, obs_point: torch.Tensor, frm_off: torch.Tensor, pt_off: torch.Tensor, pt_obs: torch.Tensor,
              frozen: torch.Tensor, frm_grp: torch.Tensor, grp_off: torch.Tensor, grp_frame: torch.Tensor, grp_params: torch.Tensor,
              grp_mask: torch.Tensor, n_points: int, n_obs: int, n_rows: int, n_groups: int, max_iters: int, loss_scale: float = 1.0,
              lam0: float = 1e-3, cg_tol: float = 1e-2, ftol: float = 1e-6) -> dict:
    """The problem of pram_bac_begin: ba_begin's with camera groups in place of per-frame parameters (include/pram_hip.h has the
    tables: frm_grp int32 [F], grp_off int32 [G + 1], grp_frame int32 [F], grp_params float64 [G, 8], grp_mask int32 [G]) -> ba_begin's
    dict, ``views`` by BAC_ARRAYS' names, ``cam=True``.  The initial cost is enqueued; nothing is read back."""
    return _ba_begin(keypoints, cam_model, None, cam_model_host, table, xyz, (obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen),
                     n_points, n_obs, n_rows, max_iters, loss_scale, lam0, cg_tol, ftol, (frm_grp, grp_off, grp_frame, grp_params, grp_mask), n_groups)


def bac_iterate(problem: dict, n_iters: int, cg_iters: int, stages: int = BA_STAGE_ALL):
    """ba_iterate on a problem of bac_begin."""
    _ba_iterate(True, problem, n_iters, cg_iters, stages)


def bac_finish(problem: dict, qvec: torch.Tensor, tvec: torch.Tensor, max_reproj_error: float = 4.0, min_tri_angle: float = 0.026179938779914945) -> dict:
    """ba_finish on a problem of bac_begin, evaluated with the refined parameters, and ``grp_params`` float64 [G, 8]: the refined
    parameters (a group that never moved keeps its input bit for bit)."""
    return _ba_finish(True, problem, qvec, tvec, max_reproj_error, min_tri_angle)


# ---- incremental mapping (csrc/mapper.hip; pram_amd/localization/mapper.py drives these) --------------------------------------
MAP_MAX_LINKS = 8      # PRAM_MAP_MAX_LINKS


def map_pair_angles(norm: torch.Tensor, frame_off: torch.Tensor, pairs: torch.Tensor, match_off: torch.Tensor, kept: torch.Tensor,
                    count: torch.Tensor, qvec: torch.Tensor, tvec: torch.Tensor, success: torch.Tensor, n_frames: int, n_pairs: int,
                    n_matches: int, workspace: Optional[torch.Tensor] = None) -> dict:
    """norm: tri_normalize with offset 0.5; pairs / match_off: the match CSR; kept int32 [M, 2], count, qvec [Pn, 4], tvec [Pn, 3],
    success int32 [Pn]: twoview_finish's -> n_tri int32 [Pn] (the kept matches whose midpoint lies in front of both cameras) and
    tri_angle float64 [Pn] (the lower median of their angles, radians; 0 for n_tri = 0)."""
    F, Pn, M = int(n_frames), int(n_pairs), int(n_matches)
    _twoview_views(norm, frame_off, pairs, match_off, kept, F, Pn, M)
    _check((count, "count", torch.int32, Pn), (qvec, "qvec", torch.float64, 4 * Pn), (tvec, "tvec", torch.float64, 3 * Pn),
           (success, "success", torch.int32, Pn))
    dev = norm.device
    workspace = _ws(int(_lib.load().pram_map_pair_angles_workspace_bytes(M)), workspace, dev, "pram_map_pair_angles: a negative number of matches")
    out = {"n_tri": _new(dev, torch.int32, Pn), "tri_angle": _new(dev, torch.float64, Pn)}
    _call("pram_map_pair_angles", norm, frame_off, pairs, match_off, kept, count, qvec, tvec, success, F, Pn, M, workspace, workspace.numel(),
          out["n_tri"], out["tri_angle"])
    return out


def map_seed(success: torch.Tensor, n_tri: torch.Tensor, tri_angle: torch.Tensor, n_pairs: int, min_num_inliers: int,
             min_tri_angle: float) -> torch.Tensor:
    """-> int32 [1]: the eligible pair (success, n_tri >= min_num_inliers, tri_angle >= min_tri_angle in radians) with the largest
    n_tri, the lowest position on a tie; -1 when none is eligible.  On the device."""
    Pn = int(n_pairs)
    _check((success, "success", torch.int32, Pn), (n_tri, "n_tri", torch.int32, Pn), (tri_angle, "tri_angle", torch.float64, Pn))
    seed = torch.empty(1, device=success.device, dtype=torch.int32)
    _call("pram_map_seed", success, n_tri, tri_angle, Pn, int(min_num_inliers), float(min_tri_angle), seed)
    return seed


def map_correspond(adj_off: torch.Tensor, adj: torch.Tensor, row_frame: torch.Tensor, n_adj: int, frame_off: torch.Tensor,
                   registered: torch.Tensor, row_point: torch.Tensor, n_frames: int, n_rows: int, n_points: int,
                   capacity: Optional[int] = None) -> dict:
    """adj_off / adj / row_frame: tri_adjacency's (n_adj: the entries adj holds); registered uint8 [F]; row_point int32 [n_rows]
    -> n_corr int32 [F], corr_off int32 [F + 1], dropped int32 [F], corr_row / corr_point int32 [capacity] ordered by (row, point).
    capacity: None sizes the lists for the worst case, min(MAP_MAX_LINKS * n_rows, n_adj)."""
    F, n, A, Pt = int(n_frames), int(n_rows), int(n_adj), int(n_points)
    _check((adj_off, "adj_off", torch.int32, n + 1), (adj, "adj", torch.int32, A), (row_frame, "row_frame", torch.int32, n),
           (frame_off, "frame_off", torch.int32, F + 1), (registered, "registered", torch.uint8, F), (row_point, "row_point", torch.int32, n))
    cap = min(MAP_MAX_LINKS * n, A) if capacity is None else int(capacity)
    dev = adj.device
    out = {"n_corr": _new(dev, torch.int32, F), "corr_off": _new(dev, torch.int32, F + 1), "dropped": _new(dev, torch.int32, F),
           "corr_row": _new(dev, torch.int32, cap), "corr_point": _new(dev, torch.int32, cap), "capacity": cap}
    _call("pram_map_correspond", adj_off, adj, row_frame, A, frame_off, registered, row_point, F, n, Pt, cap, out["n_corr"], out["corr_off"],
          out["dropped"], out["corr_row"], out["corr_point"])
    return out


def map_choose(n_corr: torch.Tensor, registered: torch.Tensor, tries: torch.Tensor, n_frames: int, min_corr: int = 30, max_reg_trials: int = 3,
               round_frames: int = 0) -> dict:
    """-> chosen int32 [F] (-1 padded), chosen_count int32 [F] and n_chosen int32 [1], on the device: the unregistered frames with
    n_corr >= min_corr and tries < max_reg_trials by (n_corr descending, frame ascending), round_frames of them at most (0: all)."""
    F = int(n_frames)
    _check((n_corr, "n_corr", torch.int32, F), (registered, "registered", torch.uint8, F), (tries, "tries", torch.int32, F))
    dev = n_corr.device
    out = {"chosen": _new(dev, torch.int32, F), "chosen_count": _new(dev, torch.int32, F), "n_chosen": _new(dev, torch.int32, 1)}
    _call("pram_map_choose", n_corr, registered, tries, F, int(min_corr), int(max_reg_trials), int(round_frames), out["chosen"], out["chosen_count"],
          out["n_chosen"])
    return out


def map_pack(chosen: torch.Tensor, n_chosen: int, corr: dict, keypoints: torch.Tensor, xyz: torch.Tensor, n_frames: int, n_rows: int,
             n_points: int, t0: int) -> dict:
    """chosen int32 [S]; corr: map_correspond's dict -> matched_keypoints float32 [S, t0, 2], matched_xyzs float64 [S, t0, 3], counts
    int32 [S] and cut int32 [S] (the rows beyond t0), as pose.estimate_poses takes them."""
    S, F, n, Pt, t0 = int(n_chosen), int(n_frames), int(n_rows), int(n_points), int(t0)
    cap = int(corr["capacity"])
    _check((chosen, "chosen", torch.int32, S), (corr["corr_off"], "corr_off", torch.int32, F + 1), (corr["corr_row"], "corr_row", torch.int32, cap),
           (corr["corr_point"], "corr_point", torch.int32, cap), (keypoints, "keypoints", torch.float32, 2 * n), (xyz, "xyz", torch.float64, 3 * Pt))
    dev = chosen.device
    out = {"matched_keypoints": _new(dev, torch.float32, S, max(t0, 1), 2), "matched_xyzs": _new(dev, torch.float64, S, max(t0, 1), 3),
           "counts": _new(dev, torch.int32, S), "cut": _new(dev, torch.int32, S)}
    _call("pram_map_pack", chosen, S, corr["corr_off"], corr["corr_row"], corr["corr_point"], cap, keypoints, xyz, F, n, Pt, t0,
          out["matched_keypoints"], out["matched_xyzs"], out["counts"], out["cut"])
    return out


def map_live_edges(edges: torch.Tensor, n_edges: int, row_frame: torch.Tensor, registered: torch.Tensor, n_frames: int, n_rows: int) -> torch.Tensor:
    """edges int32 [n_edges, 2] rows -> int32 [n_edges, 2]: the edge where the frames of both ends are registered, (-1, -1) elsewhere."""
    m, F, n = int(n_edges), int(n_frames), int(n_rows)
    _check((edges, "edges", torch.int32, 2 * m), (row_frame, "row_frame", torch.int32, n), (registered, "registered", torch.uint8, F))
    out = _new(edges.device, torch.int32, m, 2)
    _call("pram_map_live_edges", edges, m, row_frame, registered, F, n, out)
    return out


# ---- image retrieval (csrc/imgret.hip; pram_amd/localization/image_retrieval.py drives these) --------------------------------
IMGRET_DIM, IMGRET_MAX_K, IMGRET_MAX_TOPK, IMGRET_MAX_SPLITS = 128, 256, 64, 1024      # include/pram_hip.h
IMGRET_QUERY_TILE, IMGRET_DB_TILE = 32, 128      # the tile of pram_imgret_topk's grid: what a choice of ``splits`` starts from


def _imgret_rows(t: torch.Tensor, name: str) -> int:
    _chk(t, name)
    if t.dim() != 2 or t.shape[1] != IMGRET_DIM or not t.is_contiguous():
        raise _lib.PramHipError(f"{name}: expected a contiguous float32 [n, {IMGRET_DIM}] tensor, got {tuple(t.shape)}")
    return int(t.shape[0])


def imgret_assign(desc: torch.Tensor, centres: torch.Tensor):
    """desc float32 [n, 128], centres float32 [k, 128] -> (labels int32 [n]: the nearest centre, the lowest index on a tie, dist
    float64 [n]: its squared distance, summed in float64 over ascending d)."""
    n, k = _imgret_rows(desc, "desc"), _imgret_rows(centres, "centres")
    labels, dist = _new(desc.device, torch.int32, n), _new(desc.device, torch.float64, n)
    _call("pram_imgret_assign", desc, n, centres, k, labels, dist)
    return labels[:n], dist[:n]


def imgret_aggregate(desc: torch.Tensor, labels: torch.Tensor, centres: torch.Tensor, first: torch.Tensor, count: torch.Tensor):
    """The residual sums of the images first[i] .. first[i] + count[i] - 1 (int32 [n_img] row ranges into desc) -> (sums float64
    [n_img, k, 128]: per centre the sum of x - c over the image's rows with that label in ascending row index, n_assigned int32
    [n_img, k])."""
    n, k = _imgret_rows(desc, "desc"), _imgret_rows(centres, "centres")
    _check((labels, "labels", torch.int32, n), (first, "first", torch.int32), (count, "count", torch.int32))
    assert first.dim() == 1 and count.numel() == first.numel()
    m = first.numel()
    sums = _new(desc.device, torch.float64, m, max(k, 1), IMGRET_DIM)
    n_assigned = _new(desc.device, torch.int32, m, max(k, 1))
    _call("pram_imgret_aggregate", desc, labels, n, centres, k, first, count, m, sums, n_assigned)
    return sums[:m], n_assigned[:m]


def imgret_fold(sums: torch.Tensor, n_assigned: torch.Tensor, total: torch.Tensor, total_n: torch.Tensor) -> None:
    """Adds the blocks' sums float64 [n_blk, k, 128] and n_assigned int32 [n_blk, k] onto total float64 [k, 128] and total_n int32
    [k], in ascending block order."""
    _check((sums, "sums", torch.float64), (n_assigned, "n_assigned", torch.int32), (total, "total", torch.float64), (total_n, "total_n", torch.int32))
    k = int(total_n.numel())
    assert sums.dim() == 3 and sums.shape[1] == k and sums.shape[2] == IMGRET_DIM and n_assigned.numel() == sums.shape[0] * k and total.numel() == k * IMGRET_DIM
    _call("pram_imgret_fold", sums, n_assigned, int(sums.shape[0]), k, total, total_n)


def imgret_update(centres: torch.Tensor, total: torch.Tensor, total_n: torch.Tensor) -> None:
    """centres float32 [k, 128] in place: c <- float(double(c) + total / total_n) where total_n > 0."""
    k = _imgret_rows(centres, "centres")
    _check((total, "total", torch.float64), (total_n, "total_n", torch.int32))
    assert total.numel() == k * IMGRET_DIM and total_n.numel() == k
    _call("pram_imgret_update", centres, total, total_n, k)


def imgret_normalize(sums: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sums float64 [n_img, k, 128] -> the VLAD vectors float32 [n_img, k * 128] (into ``out`` when given): every centre's block
    divided by its norm, then the whole by its norm; an image without rows is all zeros."""
    _chk(sums, "sums", torch.float64)
    if sums.dim() != 3 or sums.shape[2] != IMGRET_DIM or not sums.is_contiguous():
        raise _lib.PramHipError(f"sums: expected a contiguous float64 [n_img, k, {IMGRET_DIM}] tensor, got {tuple(sums.shape)}")
    m, k = int(sums.shape[0]), int(sums.shape[1])
    if out is None:
        out = _new(sums.device, torch.float32, m, max(k, 1) * IMGRET_DIM)
    _check((out, "out", torch.float32, m * k * IMGRET_DIM))
    _call("pram_imgret_normalize", sums, m, k, out)
    return out[:m]


def imgret_topk(q: torch.Tensor, db: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None, db_valid: Optional[torch.Tensor] = None,
                splits: int = 1, workspace: Optional[torch.Tensor] = None):
    """q float32 [nq, L], db float32 [nd, L] (L a multiple of 128) -> (idx int32 [nq, k], sim float32 [nq, k]): per query the k
    database rows of largest inner product (exact fp32, one chain over L), similarity descending, then index ascending; -1 / 0 where
    fewer are allowed.  exclude int32 [nq]: an index the query may not return (-1 none); db_valid uint8 [nd]: 0 bars a row.  The
    result is the same bits for every ``splits``."""
    _chk(q, "q"), _chk(db, "db")
    if q.dim() != 2 or db.dim() != 2 or q.shape[1] != db.shape[1] or not q.is_contiguous() or not db.is_contiguous():
        raise _lib.PramHipError(f"imgret_topk: expected contiguous float32 [nq, L] and [nd, L], got {tuple(q.shape)} and {tuple(db.shape)}")
    nq, nd, Ln, k, splits = int(q.shape[0]), int(db.shape[0]), int(q.shape[1]), int(k), int(splits)
    if exclude is not None:
        _check((exclude, "exclude", torch.int32, nq))
    if db_valid is not None:
        _check((db_valid, "db_valid", torch.uint8, nd))
    need = int(_lib.load().pram_imgret_topk_workspace_bytes(nq, k, splits))
    if workspace is None:      # the process's scratch cache: retrieval asks at every query batch
        workspace = _workspace(need, q.device, "imgret_topk")
    _chk(workspace, "workspace", torch.uint8)
    idx, sim = _new(q.device, torch.int32, nq, max(k, 1)), _new(q.device, torch.float32, nq, max(k, 1))
    _call("pram_imgret_topk", q, nq, db, nd, Ln, exclude, db_valid, k, splits, workspace, workspace.numel(), idx, sim)
    return idx[:nq], sim[:nq]


# pram_amd.ops holds the stream, the pointer and check primitives and the scratch cache with its scopes; imported last, so that
# pram_amd.ops, which re-exports this module as its own last statement, finds every name above whichever of the two comes first
from .ops import _chk, _filled, _st, _workspace      # noqa: E402,F401
