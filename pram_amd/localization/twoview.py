"""Two-view geometry without poses on the device: per pair of frames an essential matrix from the matches themselves, the matches
that agree with it, and the relative pose it decomposes to (translation up to scale).

Reference: localization/triangulation.py (hloc's).
  * estimation_and_geometric_verification (triangulation.py:117-128), the ``estimate_two_view_geometries=True`` branch of main
    (triangulation.py:258-264): pycolmap.verify_matches with ransac=dict(max_num_trials=20000, min_inlier_ratio=0.1) over the
    keypoints import_features wrote (+ 0.5) -> :func:`estimate_two_view`.
:func:`keypoint_table` is the part of triangulation.frame_table that needs no poses; a frame_table result works as well, the
estimator reads none of its pose-dependent keys.  The kernels are csrc/twoview.hip: a five-point sampler and solver
per (pair, trial), a (hypotheses x matches) Sampson scoring pass, and per pair the decomposition, a 5-DoF Levenberg-Marquardt and
the outputs in pram_tri_verify's layout, so that triangulation.triangulate_map(estimate_two_view_geometries=True) runs its stages
2b to 4 on them unchanged.  torch here is plumbing: uploads, the walk over the pairs in chunks of ``pair_chunk`` (the workspace of
ops.TWOVIEW_TRIAL_BYTES per trial depends on the chunk, not on the map; the result does not depend on the chunk) and one read-back
at the end.  profiles/twoview_timing.md has the time of every stage.

Where this differs from the reference, on purpose:
  * not COLMAP's estimator, and parity with pycolmap is not claimed (pycolmap was never run beside this).  The inlier threshold
    max_error * 0.5 * (1 / f0 + 1 / f1) on the normalised plane is COLMAP's rule as remembered, not verified.
  * the trial budget is fixed: ``trials`` five-point samples per pair (1024 miss an all-inlier sample with probability below 1e-4
    for inlier ratios from about 0.4), where the reference allows 20000 adaptive trials.  Below 0.4 the caller raises ``trials``.
  * only the calibrated configuration is estimated: no fundamental matrix, no homography, and no classification of a pair as
    planar, panoramic or watermark.
  * a pure rotation leaves the translation undetermined: ``qvec`` and the mask are still meaningful, ``tvec`` is not, and
    ``num_front`` does not say so; mapper.initial_pairs' ``tri_angle`` does.
  * no local optimisation inside the loop: the best hypothesis is refined once the loop is over.
  * out-of-range indices: a match with a keypoint index outside its frame is no inlier and a sample that draws it yields no
    hypothesis, where the reference would raise."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import triangulation as tri

TWOVIEW_DEFAULTS = dict(max_error=4.0, trials=1024, seed=0, min_inlier_ratio=0.1, min_num_inliers=15, refine_iters=20, pair_chunk=256)
_PAIR_KEYS = ("E", "qvec", "tvec", "num_inliers", "num_front", "success")


@torch.no_grad()
def keypoint_table(frames: Sequence[dict], cameras: Sequence, device) -> dict:
    """frames: dicts with ``keypoints`` [n, 2] or [n, 3]; cameras: one (model_name, width, height, params) tuple per frame -> the
    pose-free part of triangulation.frame_table: keypoints, frame_off, the cameras and ``norm05`` (keypoint + 0.5 through the
    inverse camera model), on the device."""
    from pram_amd.localization.pose import camera_table
    device = tri._device(device)
    F = len(frames)
    if len(cameras) != F:
        raise ValueError(f"keypoint_table: {F} frames need {F} cameras")
    ids, prm = camera_table(cameras)
    lens = [int(np.asarray(f["keypoints"]).shape[0]) for f in frames]
    if sum(lens) > 2 ** 30:
        raise ValueError("keypoint_table: more than 2^30 keypoints")
    frame_off = np.zeros(F + 1, dtype=np.int32)
    frame_off[1:] = np.cumsum(lens)
    kp = [np.asarray(f["keypoints"], dtype=np.float32).reshape(n, -1)[:, :2] for f, n in zip(frames, lens) if n]
    kp = np.concatenate(kp) if kp else np.zeros((0, 2), dtype=np.float32)
    n_rows = int(frame_off[-1])
    t = {"n_frames": F, "n_rows": n_rows, "frame_off_host": frame_off, "cam_model_host": ids.tolist(), "keypoints": tri._up(kp, device),
         "frame_off": tri._up(frame_off, device), "cam_model": tri._up(ids, device), "cam_params": tri._up(prm, device)}
    t["norm05"] = ops.tri_normalize(t["keypoints"], t["frame_off"], t["cam_model"], t["cam_params"], t["cam_model_host"], n_rows, 0.5)
    return t


def _twoview_params(name: str, params: dict) -> dict:
    p = tri._params(name, params, TWOVIEW_DEFAULTS)
    for k in ("trials", "pair_chunk"):
        if int(p[k]) != p[k] or p[k] < 1:
            raise ValueError(f"{k}: an integer >= 1")
        p[k] = int(p[k])
    return tri._int_param(tri._int_param(p, "min_num_inliers"), "refine_iters")


@torch.no_grad()
def _estimate(table: dict, pairs, matches, p: dict) -> dict:
    """Everything on the device: tri._verify's dict (keep, kept, edges, count, pair_index, pairs, match_off, n_matches) plus the
    per-pair results."""
    use, pr, off, flat = tri._match_csr(table, pairs, matches)
    dev = table["keypoints"].device
    Pn, M, F = len(use), flat.shape[0], table["n_frames"]
    d_pairs, d_off, d_flat = tri._up(pr, dev), tri._up(off, dev), tri._up(flat, dev)
    out = ops.twoview_outputs(Pn, M, dev)
    views = (table["norm05"], table["frame_off"])
    for a in range(0, Pn, p["pair_chunk"]):      # the hypotheses of a chunk are dead once the chunk is finished
        b = min(a + p["pair_chunk"], Pn)
        cp, co = d_pairs[a:b], d_off[a:b + 1]
        h = ops.twoview_hypotheses(*views, cp, co, d_flat, F, b - a, M, first_pair=a, trials=p["trials"], seed=p["seed"])
        s = ops.twoview_score(*views, cp, co, d_flat, table["cam_model"], table["cam_params"], F, b - a, M, h["E"], h["n_sol"], p["max_error"])
        cut = {k: (out[k][a:b] if k in _PAIR_KEYS or k == "count" else out[k]) for k in out}
        ops.twoview_finish(*views, cp, co, d_flat, table["cam_model"], table["cam_params"], F, b - a, M, h["E"], s["h_inliers"], s["best"],
                           max_error=p["max_error"], min_inlier_ratio=p["min_inlier_ratio"], min_num_inliers=p["min_num_inliers"],
                           refine_iters=p["refine_iters"], out=cut)
    out.update(pair_index=use, pairs=pr, match_off=off, n_matches=M)
    return out


def _pair_results(v: dict) -> dict:
    Pn = len(v["pair_index"])
    res = {k: v[k][:Pn].cpu().numpy() for k in _PAIR_KEYS}
    res["success"] = res["success"].astype(bool)
    return res


def estimate_two_view(table: dict, pairs, matches: Sequence, **params) -> dict:
    """table: :func:`keypoint_table` (or triangulation.frame_table); pairs [Pn, 2] frame indices; matches: per pair int [m, 2]
    (keypoint index in frame 0, in frame 1) -> on the host ``pair_index``, ``keep``, ``kept`` and ``inlier_ratio`` shaped as
    triangulation.verify_matches gives them, plus per processed pair ``E`` float64 [Pn, 9] (row-major, x1^T E x0 = 0 on the
    normalised plane, Frobenius norm 1), ``qvec`` [Pn, 4] (w, x, y, z) and ``tvec`` [Pn, 3] (unit) of frame 1 from frame 0,
    ``num_inliers``, ``num_front`` (the inliers at positive depth in both frames) and ``success`` (bool).  A failed pair has zeros
    everywhere and keeps no match.  params: TWOVIEW_DEFAULTS."""
    p = _twoview_params("estimate_two_view", params)
    v = _estimate(table, pairs, matches, p)
    M, off, Pn = v["n_matches"], v["match_off"], len(v["pair_index"])
    keep, kept, count = v["keep"][:M].cpu().numpy().astype(bool), v["kept"][:M].cpu().numpy(), v["count"][:Pn].cpu().numpy()
    return {"pair_index": v["pair_index"], "keep": [keep[a:b] for a, b in zip(off[:-1], off[1:])],
            "kept": [kept[a:a + c] for a, c in zip(off[:-1], count)], "inlier_ratio": tri._inlier_ratio(count, off), **_pair_results(v)}
