"""Incremental mapping on the device: poses and points from images' keypoints and pairwise matches alone, the step that makes
triangulation.triangulate_map and bundle.bundle_adjust usable on data without poses.

Reference: the reference has no such stage: its README sends data without good poses "through COLMAP" before its own
localization/triangulation.py runs.  pycolmap is not installed here and was never run beside this, so nothing is pinned to it;
the seed thresholds (init_min_num_inliers 100, init_min_tri_angle 16 degrees) and the absolute-pose thresholds (abs_pose_max_error
12 px, abs_pose_min_num_inliers 30, abs_pose_min_inlier_ratio 0.25) are COLMAP's defaults as remembered, not verified.
  * :func:`reconstruct` runs everything and returns triangulate_map's dict plus the poses.
  * :func:`initial_pairs`, :func:`correspondences`, :func:`choose_frames`: one stage each, results on the host.
  * :func:`similarity_from_centres`, :func:`apply_similarity`: a map is recovered up to a similarity; with a few known camera
    positions these two (numpy, on the host) bring it into the caller's metric frame.

The stages (csrc/mapper.hip has the new kernels, DESIGN.md 4.26 the formulas):
  0. twoview._estimate over all unique pairs, unchanged, and pram_tri_adjacency over its edges, once.
  1. pram_map_pair_angles: per pair the kept matches that its relative pose triangulates in front of both cameras (``n_tri``) and
     the lower median of their triangulation angles (``tri_angle``); pram_map_seed: the pair with the largest n_tri among those
     with success, n_tri >= init_min_num_inliers and tri_angle >= init_min_tri_angle; both thresholds are halved up to
     ``init_relax`` times when no pair is eligible.  A pure rotation has a small tri_angle whatever its number of matches.
  2. The seed's first frame (the one with the lower index) is the world: identity; the other gets the pair's relative pose, so
     the seed baseline has length 1.
  3. pram_map_correspond: for every keypoint of an unregistered frame the points of the current model that its matches in
     registered frames carry.
  4. pram_map_choose picks the frames with ``min_corr`` correspondences at least that were tried fewer than ``max_reg_trials``
     times, pram_map_pack lays their lists out, pose.estimate_poses (seg_k=1, threshold ``abs_pose_max_error``, 1000 trials, seed
     ``seed + round``) solves them all at once, and a frame is accepted on success with num_inliers >=
     abs_pose_min_num_inliers and >= abs_pose_min_inlier_ratio * count.
  5. pram_map_live_edges keeps the matches between registered frames; triangulation's stage 2b (with ``min_support`` > 0), tracks
     and stage 4 run on them with the current poses, then bundle.py's solve for ``ba_iters`` iterations with the seed's first
     frame frozen, of its second the translation component of largest magnitude (which fixes the scale) and every unregistered
     frame; the adjusted poses and the filtered points are what the next round's stage 3 reads.
The rounds end when a round chooses no frame or after ``max_rounds``; then one more triangulation with the final poses and one
bundle_adjust with ``final_ba_iters`` give the result.  That last triangulation starts from the two-view stage's matches that also
pass triangulation's own epipolar test against the final poses (``max_error`` pixels): an estimated E lets wrong matches near its
epipolar lines through, the recovered poses do not; a pair without a baseline (``tri_angle`` under the triangulation's
``min_tri_angle``: a pure rotation) keeps the two-view stage's matches.

torch here is plumbing.  Host synchronisations per round: the choice (one small read-back), the acceptance (one), the
triangulation's own (the components' done flag once per triangulation.CC_GROUP rounds, the track table's sizes), the sizes of the
observation tables (three), the adjuster's done word once per bundle.BA_GROUP iterations and one read of its state.  There is no
per-frame and no per-point loop on the host before the final tables, which are triangulation._tables' and bundle.clean_model's.
Nothing about this stage's speed has been measured beyond profiles/mapper_timing.md's one run.

Where this differs from COLMAP's incremental mapper, on purpose:
  * every eligible frame of a round is registered at once against the same points; COLMAP registers one image at a time;
  * the model is re-triangulated in full and adjusted globally every round: no local bundle adjustment;
  * no Merge, Complete or Retriangulate; intrinsics stay constant; every budget is fixed;
  * one connected component only: what stays unregistered gets no second seed; a seed is never abandoned once chosen;
  * the thresholds are COLMAP's as remembered (above)."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import bundle, pose, twoview
from pram_amd.localization import triangulation as tri

MAP_DEFAULTS = dict(init_min_num_inliers=100, init_min_tri_angle=16.0, init_relax=2, min_corr=30, max_reg_trials=3, round_frames=0,
                    max_corr=4096, abs_pose_max_error=12.0, abs_pose_min_num_inliers=30, abs_pose_min_inlier_ratio=0.25, max_rounds=50,
                    ba_iters=10, final_ba_iters=bundle.BA_DEFAULTS["max_iters"], min_support=0, max_error=tri.VERIFY_DEFAULTS["max_error"], seed=0, twoview=None, triangulation=None,
                    bundle=None)
POSE_TRIALS = 1000
REASONS = ("no_correspondences", "few_correspondences", "pose_failed", "max_rounds")
_BA_OWN = ("max_iters", "gauge", "frozen")      # what the mapper sets itself


def _map_params(name: str, params: dict) -> dict:
    p = tri._params(name, params, MAP_DEFAULTS)
    for k in ("init_min_num_inliers", "init_relax", "min_corr", "max_reg_trials", "round_frames", "abs_pose_min_num_inliers", "max_rounds",
              "ba_iters", "final_ba_iters", "min_support"):
        p = tri._int_param(p, k)
    if int(p["max_corr"]) != p["max_corr"] or not 4 <= p["max_corr"] <= 2 ** 20:
        raise ValueError("max_corr: an integer in [4, 2^20]")
    p["max_corr"] = int(p["max_corr"])
    for k in ("init_min_tri_angle", "abs_pose_max_error", "abs_pose_min_inlier_ratio"):
        if not np.isfinite(float(p[k])) or p[k] < 0:
            raise ValueError(f"{k}: finite and >= 0")
    if not p["abs_pose_max_error"] > 0 or not (np.isfinite(float(p["max_error"])) and p["max_error"] > 0):
        raise ValueError("abs_pose_max_error, max_error: finite and > 0")
    if p["init_relax"] > 30:
        raise ValueError("init_relax: at most 30")
    p["twoview"] = twoview._twoview_params(f"{name}: twoview", dict(p["twoview"] or {}))
    p["triangulation"] = tri._params(f"{name}: triangulation", dict(p["triangulation"] or {}), tri.TRI_DEFAULTS)
    own = set(p["bundle"] or {}) & set(_BA_OWN)
    if own:
        raise ValueError(f"bundle: {sorted(own)} are the mapper's (ba_iters, final_ba_iters)")
    p["bundle"] = bundle._ba_params(f"{name}: bundle", dict(p["bundle"] or {}))
    return p


# ------------------------------------------------------------------ the two host utilities
def _rot(q: np.ndarray) -> np.ndarray:
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def _qvec(R: np.ndarray) -> np.ndarray:
    """Rotation matrix -> (w, x, y, z) with w >= 0, by the largest of the four squared components."""
    t = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(t))
    q = np.array([[t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], [R[2, 1] - R[1, 2], t[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
                  [R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], t[2], R[1, 2] + R[2, 1]], [R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], t[3]]])[k]
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def centres(qvecs, tvecs) -> np.ndarray:
    """cam_from_world poses -> the cameras' centres -R^T t, float64 [F, 3]."""
    qv, tv = np.asarray(qvecs, dtype=np.float64).reshape(-1, 4), np.asarray(tvecs, dtype=np.float64).reshape(-1, 3)
    return np.stack([-_rot(q).T @ t for q, t in zip(qv, tv)]) if len(qv) else np.zeros((0, 3))


def similarity_from_centres(src, dst) -> tuple:
    """Umeyama's closed form: (s, R, t) minimising sum |dst - (s R src + t)|^2 over similarities; src, dst float [n, 3], n >= 3 and
    not collinear.  R is a rotation (det +1)."""
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    if src.shape != dst.shape or src.shape[0] < 3:
        raise ValueError("similarity_from_centres: two arrays [n, 3] with n >= 3")
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    var = (a * a).sum() / len(a)
    if not var > 0:
        raise ValueError("similarity_from_centres: the source points coincide")
    U, D, Vt = np.linalg.svd(b.T @ a / len(a))
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ np.diag(S) @ Vt
    s = float((D * S).sum() / var)
    return s, R, md - s * R @ ms


def apply_similarity(result: dict, s: float, R, t) -> dict:
    """:func:`reconstruct`'s dict (or any model dict with ``qvecs`` / ``tvecs``) with world points X moved to s R X + t: the points,
    the frames' ``xyzs`` (where a keypoint has a point) and the poses of the registered frames (every frame when the dict has no
    ``registered``).  A new dict; the input is not modified."""
    R, t, s = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3), float(s)
    out = dict(result)
    out["point3D_xyzs"] = s * np.asarray(result["point3D_xyzs"], dtype=np.float64).reshape(-1, 3) @ R.T + t
    if "frames" in result:
        out["frames"] = [{**f, "xyzs": np.where((np.asarray(f["point3D_ids"]) >= 0)[:, None], s * np.asarray(f["xyzs"]).reshape(-1, 3) @ R.T + t, 0.0)}
                         for f in result["frames"]]
    qv, tv = np.array(result["qvecs"], dtype=np.float64), np.array(result["tvecs"], dtype=np.float64)
    reg = np.asarray(result["registered"]).astype(bool) if "registered" in result else np.ones(len(qv), dtype=bool)
    for f in np.nonzero(reg)[0].tolist():
        Rc = _rot(qv[f]) @ R.T
        qv[f], tv[f] = _qvec(Rc), s * tv[f] - Rc @ t
    out["qvecs"], out["tvecs"] = qv, tv
    return out


# ------------------------------------------------------------------ stages 0 and 1
@torch.no_grad()
def _scores(table: dict, v: dict) -> dict:
    Pn = len(v["pair_index"])
    dev = table["keypoints"].device
    return ops.map_pair_angles(table["norm05"], table["frame_off"], tri._up(v["pairs"], dev), tri._up(v["match_off"], dev), v["kept"], v["count"],
                               v["qvec"], v["tvec"], v["success"], table["n_frames"], Pn, v["n_matches"])


@torch.no_grad()
def _seed(v: dict, sc: dict, p: dict) -> tuple:
    """-> (the seed's position among the processed pairs or -1, the halvings it took); one int read back per call."""
    Pn = len(v["pair_index"])
    for k in range(p["init_relax"] + 1):
        s = int(ops.map_seed(v["success"], sc["n_tri"], sc["tri_angle"], Pn, p["init_min_num_inliers"] >> k,
                             float(np.deg2rad(p["init_min_tri_angle"])) / 2 ** k).item())
        if s >= 0:
            return s, k
    return -1, p["init_relax"]


def _two_view(v: dict, sc: dict) -> dict:
    Pn = len(v["pair_index"])
    return {**twoview._pair_results(v), "n_tri": sc["n_tri"][:Pn].cpu().numpy(), "tri_angle": sc["tri_angle"][:Pn].cpu().numpy()}


def initial_pairs(table: dict, pairs, matches: Sequence, **params) -> dict:
    """Stages 0 and 1 on their own.  table: twoview.keypoint_table; pairs, matches: triangulate_map's -> on the host
    twoview.estimate_two_view's per-pair results plus ``n_tri`` int32 and ``tri_angle`` float64 (radians) per processed pair,
    ``pair_index``, ``seed_pair`` (a position in pair_index, -1: none) and ``relaxed`` (the halvings of the thresholds it took).
    params: init_min_num_inliers, init_min_tri_angle (degrees), init_relax, twoview."""
    p = _map_params("initial_pairs", params)
    v = twoview._estimate(table, pairs, matches, p["twoview"])
    sc = _scores(table, v)
    seed, relaxed = _seed(v, sc, p)
    return {**_two_view(v, sc), "pair_index": v["pair_index"], "seed_pair": seed, "relaxed": relaxed}


# ------------------------------------------------------------------ stages 3 and 4
def correspondences(table: dict, edges, registered, row_point, n_points: int) -> dict:
    """Stage 3 on its own.  edges: int [n, 2] rows joined by a kept match; registered: bool [F]; row_point: int [n_rows], a row's
    point in the model or -1 -> on the host ``n_corr`` int32 [F], ``corr_off`` int32 [F + 1], ``corr_row`` / ``corr_point`` int32
    [corr_off[-1]] ordered by (row, point), and ``dropped`` int32 [F]."""
    dev, F, n = table["keypoints"].device, table["n_frames"], table["n_rows"]
    e = tri._edges(edges)
    reg, rp = np.asarray(registered).astype(np.uint8).reshape(-1), np.asarray(row_point).astype(np.int32).reshape(-1)
    if reg.shape[0] != F or rp.shape[0] != n:
        raise ValueError(f"correspondences: registered [{F}] and row_point [{n}]")
    a = ops.tri_adjacency(tri._up(e, dev), e.shape[0], table["frame_off"], F, n)
    c = ops.map_correspond(a["adj_off"], a["adj"], a["row_frame"], 2 * e.shape[0], table["frame_off"], tri._up(reg, dev), tri._up(rp, dev), F, n,
                           int(n_points))
    off = c["corr_off"][:F + 1].cpu().numpy()
    return {"n_corr": c["n_corr"][:F].cpu().numpy(), "corr_off": off, "dropped": c["dropped"][:F].cpu().numpy(),
            "corr_row": c["corr_row"][:int(off[-1])].cpu().numpy(), "corr_point": c["corr_point"][:int(off[-1])].cpu().numpy()}


def choose_frames(n_corr, registered, tries, device, **params) -> tuple:
    """Stage 4's choice on its own -> (frames int32 [S], their n_corr int32 [S]) on the host, ordered by (n_corr descending, frame
    ascending).  params: min_corr, max_reg_trials, round_frames."""
    p = _map_params("choose_frames", params)
    dev = tri._device(device)
    nc, reg, tr = (np.asarray(a).reshape(-1) for a in (n_corr, registered, tries))
    if not nc.shape == reg.shape == tr.shape:
        raise ValueError("choose_frames: n_corr, registered and tries of one length")
    ch = ops.map_choose(tri._up(nc.astype(np.int32), dev), tri._up(reg.astype(np.uint8), dev), tri._up(tr.astype(np.int32), dev), nc.shape[0],
                        p["min_corr"], p["max_reg_trials"], p["round_frames"])
    S = int(ch["n_chosen"].item())
    return ch["chosen"][:S].cpu().numpy(), ch["chosen_count"][:S].cpu().numpy()


# ------------------------------------------------------------------ stage 5
@torch.no_grad()
def _triangulate(table: dict, v: dict, adj: dict, reg: torch.Tensor, qv: torch.Tensor, tv: torch.Tensor, p: dict, n_reg: int,
                 source: torch.Tensor = None) -> tuple:
    """The matches between registered frames through stages 2b to 4 at the current poses -> (track table, stage 4's results).  Stage
    2b asks for a third view, so it runs from three registered frames (``n_reg``) on: the seed pair alone has none.  ``source``:
    the edges to start from instead of the two-view stage's (the finish's, :func:`_verified`)."""
    M = v["n_matches"]
    edges = ops.map_live_edges(v["edges"] if source is None else source, M, adj["row_frame"], reg, table["n_frames"], table["n_rows"])
    table["frames"] = ops.tri_frames(qv, tv, table["cam_model"], table["cam_params"], table["cam_model_host"])
    tp = {**p["triangulation"], "min_support": p["min_support"]}
    if p["min_support"] > 0 and n_reg >= 3:
        edges = tri._support(table, edges, M, tp)["edges"]
    t = tri._tracks(table, edges, M)
    return t, tri._triangulate(table, t, tp)


@torch.no_grad()
def _verified(table: dict, v: dict, sc: dict, pairs, matches, qv: torch.Tensor, tv: torch.Tensor, p: dict) -> torch.Tensor:
    """The finish's edges: the two-view stage's, of which a match stays only when it also passes triangulation's own stage 2, the
    epipolar test against the poses (now that there are poses: ``max_error`` pixels, keypoints at offset 0, as triangulate_map
    tests them).  An estimated E lets a wrong match near its epipolar line through; the recovered poses of the two frames do not
    have that freedom.  A pair whose ``tri_angle`` is below the triangulation's ``min_tri_angle`` has no baseline to speak of and
    so no epipolar geometry to test against (a pure rotation): its matches stay as the two-view stage left them."""
    dev, M, Pn = table["keypoints"].device, v["n_matches"], len(v["pair_index"])
    if M == 0:
        return v["edges"]
    if "norm0" not in table:
        table["norm0"] = ops.tri_normalize(table["keypoints"], table["frame_off"], table["cam_model"], table["cam_params"], table["cam_model_host"],
                                           table["n_rows"], 0.0)
    table["frames"] = ops.tri_frames(qv, tv, table["cam_model"], table["cam_params"], table["cam_model_host"])
    ver = tri._verify(table, pairs, matches, p["max_error"])["edges"][:M]
    match_pair = tri._up(np.repeat(np.arange(Pn), np.diff(v["match_off"])), dev)
    flat = (sc["tri_angle"][:Pn] < float(np.deg2rad(p["triangulation"]["min_tri_angle"])))[match_pair]
    keep = (ver[:, 0] >= 0) | flat
    out = v["edges"].clone()
    out[:M] = torch.where(keep[:, None], v["edges"][:M], torch.full_like(ver, -1))
    return out


@torch.no_grad()
def _adjust(table: dict, t: dict, out: dict, frozen: torch.Tensor, qv: torch.Tensor, tv: torch.Tensor, p: dict, iters: int) -> dict:
    """bundle.py's solve on the accepted tracks, the observation tables built on the device -> the adjusted poses, the points, every
    row's point (the filter applied) and the figures of the report."""
    dev, F, n = table["keypoints"].device, table["n_frames"], table["n_rows"]
    T, E = t["n_tracks"], t["n_entries"]
    none = {"qv": qv, "tv": tv, "xyz": torch.zeros(1, 3, device=dev, dtype=torch.float64), "n_points": 0,
            "row_point": torch.full((max(n, 1),), -1, device=dev, dtype=torch.int32), "points": 0, "observations": 0, "termination": "empty",
            "initial_cost": 0.0, "final_cost": 0.0, "lm_iterations": 0}
    if T == 0 or E == 0:
        return none
    accept = out["accept"][:T] != 0
    lens = (t["trk_off"][1:T + 1] - t["trk_off"][:T]).long()
    trk_of = torch.repeat_interleave(torch.arange(T, device=dev), lens, output_size=E)
    use = accept[trk_of] & (out["entry_keep"][:E] != 0)
    pidx = torch.cumsum(accept.int(), 0) - 1
    rows, pts, frm = t["trk_row"][:E][use], pidx[trk_of][use], t["trk_frame"][:E][use]
    xyz = out["xyz"][:T][accept].contiguous()
    Pn, O = int(xyz.shape[0]), int(rows.shape[0])
    if Pn == 0 or O == 0:
        return none
    order = torch.argsort(rows)      # a row is in one track: the order is unique
    obs_row, obs_point, obs_frame = (a[order].to(torch.int32).contiguous() for a in (rows, pts, frm))
    frm_off = torch.searchsorted(obs_row, table["frame_off"][:F + 1].contiguous()).to(torch.int32)
    pt_off = torch.zeros(Pn + 1, device=dev, dtype=torch.int32)
    pt_off[1:] = torch.cumsum(torch.bincount(obs_point.long(), minlength=Pn), 0)
    pt_obs = torch.argsort(obs_point, stable=True).to(torch.int32)
    b = p["bundle"]
    prob = ops.ba_begin(table["keypoints"], table["cam_model"], table["cam_params"], table["cam_model_host"], table["frames"], xyz, obs_row,
                        obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen, Pn, O, n, iters, loss_scale=b["loss_scale"], lam0=b["lam0"],
                        cg_tol=b["cg_tol"], ftol=b["ftol"])
    state = prob["views"]["state_i32"]
    for _ in range(0, iters, bundle.BA_GROUP):
        ops.ba_iterate(prob, bundle.BA_GROUP, b["cg_iters"])
        if int(state[ops.BA_SI_DONE].item()):
            break
    fin = ops.ba_finish(prob, qv, tv, max_reproj_error=b["max_reproj_error"], min_tri_angle=float(np.deg2rad(b["min_tri_angle"])))
    stays = (fin["obs_keep"] != 0) & (fin["pt_keep"][obs_point.long()] != 0)
    row_point = torch.full((max(n, 1),), -1, device=dev, dtype=torch.int32)
    row_point[obs_row[stays].long()] = obs_point[stays]
    sd = prob["views"]["state_f64"]
    fig = torch.cat([sd[ops.BA_SD_COST0:ops.BA_SD_COST0 + 1], sd[ops.BA_SD_COST:ops.BA_SD_COST + 1], state[:ops.BA_STATE_I32].double(),
                     (fin["pt_keep"] != 0).sum().double().reshape(1)]).cpu().numpy()
    si = fig[2:2 + ops.BA_STATE_I32].astype(np.int64)
    reason = ops.BA_REASONS.get(int(si[ops.BA_SI_REASON]), "unknown")
    if reason == "tables":
        raise ops._lib.PramHipError("reconstruct: the observation tables failed the check on the device")
    return {"qv": fin["qvec"], "tv": fin["tvec"], "xyz": fin["xyz"], "n_points": Pn, "row_point": row_point, "points": int(fig[-1]),
            "observations": O, "termination": reason if iters else "filter_only", "initial_cost": float(fig[0]), "final_cost": float(fig[1]),
            "lm_iterations": int(si[ops.BA_SI_LM_ITER])}


def _empty_model(frame_ids, frame_off) -> dict:
    z = np.zeros(0, dtype=np.int32)
    return tri._tables(frame_ids, frame_off, [({"trk_off": np.zeros(1, dtype=np.int32), "trk_row": z, "trk_frame": z, "trk_kpt": z},
                                                {"accept": z, "entry_keep": z, "xyz": np.zeros((0, 3)), "error": np.zeros(0)})])[0]


# ------------------------------------------------------------------ the mapper
@torch.no_grad()
def reconstruct(frames: Sequence[dict], cameras: Sequence, pairs, matches: Sequence, device, **params) -> dict:
    """frames, cameras: twoview.keypoint_table's (dicts with ``keypoints``; one (model_name, width, height, params) tuple per frame);
    pairs [Pn, 2] positions in ``frames`` and matches, per pair int [m, 2]: triangulation.triangulate_map's -> a dict with every key
    of triangulate_map's (``point_ids``, ``point3D_xyzs``, ``track_error``, ``tracks``, ``point3D_frame_ids``, ``frames``,
    ``pair_index``, ``inlier_ratio``) over all frames, a frame that was not registered having no points, so that
    bundle.bundle_adjust, labelling.label_points, mapbuild.build_store_inputs and DatabaseStore.from_triangulation take it as it
    is, plus
      ``qvecs`` float64 [F, 4] (w, x, y, z) and ``tvecs`` [F, 3]: cam_from_world, identity and zero for an unregistered frame;
      ``registered`` bool [F]; ``frame_round`` int32 [F] (-1: never registered, 0: the seed pair, r: round r);
      ``seed_pair``: a position in ``pair_index``, -1 without a seed;
      ``two_view``: twoview.estimate_two_view's per-pair results plus ``n_tri`` and ``tri_angle`` (radians);
      ``report``: ``success``, ``reason`` (None or 'no_seed'), ``seed_frames``, ``seed_relaxed``, ``rounds`` (per round a dict:
      ``frames_tried``, ``frames_accepted``, ``correspondences``, ``cut`` (rows beyond max_corr), ``points``, ``observations``,
      ``ba_termination``, ``ba_initial_cost``, ``ba_final_cost``, ``ba_iterations``; round 0 is the seed's), ``unregistered``
      (frame -> one of REASONS, as the last look at the correspondences found it: after ``max_rounds`` a frame whose neighbours
      are not registered yet has 'no_correspondences') and ``final_ba`` (bundle_adjust's report);
      ``cameras`` and ``camera_groups``: bundle_adjust's, one (model_name, width, height, params) tuple per frame.
    Intrinsics.  ``bundle=dict(refine_focal_length=True, ...)`` (bundle.BA_DEFAULTS' three refine flags and ``camera_groups``)
    reaches the final adjustment, which refines the camera groups' parameters and returns them as ``cameras``.  The per-round
    solves ignore the flags and keep the intrinsics constant: they share the round's frame table, whose normalised keypoints come
    from the input cameras.  So a caller with a rough focal length runs ``reconstruct`` again with the returned ``cameras``, so
    that the two-view and P3P stages see them, and gives ``result['cameras']`` (not the input cameras) to
    DatabaseStore.from_triangulation and triangulation.frame_table.
    World frame and scale: the camera frame of the seed's first frame, the seed baseline of length 1.  Without an eligible pair
    ``report['success']`` is False, the reason 'no_seed' and the model empty; nothing is raised.  params: MAP_DEFAULTS
    (``twoview``, ``triangulation``, ``bundle``: dicts of twoview.TWOVIEW_DEFAULTS', triangulation.TRI_DEFAULTS' and
    bundle.BA_DEFAULTS' parameters).  The module docstring has the stages, the host synchronisations and the deviations."""
    p = _map_params("reconstruct", params)
    table = twoview.keypoint_table(frames, cameras, device)
    dev, F, n = table["keypoints"].device, table["n_frames"], table["n_rows"]
    frame_ids = np.array([f.get("id", i) for i, f in enumerate(frames)])
    v = twoview._estimate(table, pairs, matches, p["twoview"])
    Pn, M = len(v["pair_index"]), v["n_matches"]
    sc = _scores(table, v)
    seed, relaxed = _seed(v, sc, p)
    two_view = _two_view(v, sc)
    qv, tv = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (F, 1)), np.zeros((F, 3))
    res_tail = {"pair_index": v["pair_index"], "inlier_ratio": tri._inlier_ratio(v["count"][:Pn].cpu().numpy(), v["match_off"]), "two_view": two_view}
    if seed < 0:
        res = _empty_model(frame_ids, table["frame_off_host"])
        res.update(res_tail, qvecs=qv, tvecs=tv, registered=np.zeros(F, dtype=bool), frame_round=np.full(F, -1, dtype=np.int32), seed_pair=-1,
                   removed_ids=np.zeros(0, dtype=np.int64), cameras=list(cameras), camera_groups=bundle.camera_groups(cameras, p["bundle"]["camera_groups"]),
                   report={"success": False, "reason": "no_seed", "seed_frames": None, "seed_relaxed": relaxed, "rounds": [],
                           "unregistered": {f: "no_correspondences" for f in range(F)}, "final_ba": None})
        return res
    # ---- stage 2: the seed's frames
    f0, f1 = (int(x) for x in v["pairs"][seed])
    q01, t01 = two_view["qvec"][seed], two_view["tvec"][seed]
    a, b = min(f0, f1), max(f0, f1)
    if b == f0:      # the pair gives f1 from f0: invert it
        R = _rot(q01)
        q01, t01 = np.array([q01[0], -q01[1], -q01[2], -q01[3]]), -R.T @ t01
    qv[b], tv[b] = q01, t01
    frozen = np.full(F, bundle.FROZEN_ALL, dtype=np.int32)
    frozen_b = 1 << (3 + int(np.argmax(np.abs(t01))))
    adj = ops.tri_adjacency(v["edges"], M, table["frame_off"], F, n)
    reg = torch.zeros(max(F, 1), device=dev, dtype=torch.uint8)
    reg[[a, b]] = 1
    tries = torch.zeros(max(F, 1), device=dev, dtype=torch.int32)
    fround = torch.full((max(F, 1),), -1, device=dev, dtype=torch.int32)
    fround[[a, b]] = 0
    qv_d, tv_d = tri._up(qv, dev), tri._up(tv, dev)

    def grow(iters: int) -> dict:
        mask = torch.where(reg[:F] != 0, 0, bundle.FROZEN_ALL).to(torch.int32)
        mask[a], mask[b] = bundle.FROZEN_ALL, frozen_b
        t, out = _triangulate(table, v, adj, reg, qv_d, tv_d, p, n_reg)
        return _adjust(table, t, out, mask.contiguous(), qv_d, tv_d, p, iters)

    def line(m: dict, tried, accepted, corr, cut) -> dict:
        return {"frames_tried": tried, "frames_accepted": accepted, "correspondences": corr, "cut": cut, "points": m["points"],
                "observations": m["observations"], "ba_termination": m["termination"], "ba_initial_cost": m["initial_cost"],
                "ba_final_cost": m["final_cost"], "ba_iterations": m["lm_iterations"]}

    n_reg = 2
    m = grow(p["ba_iters"])
    qv_d, tv_d = m["qv"], m["tv"]
    rounds = [line(m, [a, b], [a, b], 0, 0)]
    rnd = 0
    while True:
        corr = ops.map_correspond(adj["adj_off"], adj["adj"], adj["row_frame"], 2 * M, table["frame_off"], reg, m["row_point"], F, n, m["n_points"])
        ch = ops.map_choose(corr["n_corr"], reg, tries, F, p["min_corr"], p["max_reg_trials"], p["round_frames"])
        host = torch.cat([ch["n_chosen"], ch["chosen"][:F], ch["chosen_count"][:F]]).cpu().numpy()      # the round's read-back before the pose stage
        S = int(host[0])
        if S == 0 or rnd >= p["max_rounds"]:
            break
        rnd += 1
        chosen, counts = host[1:1 + S], host[1 + F:1 + F + S]
        pk = ops.map_pack(ch["chosen"], S, corr, table["keypoints"], m["xyz"], F, n, m["n_points"], min(int(counts.max()), p["max_corr"]))
        idx = ch["chosen"][:S].long()
        cams = (table["cam_model"][idx].contiguous(), table["cam_params"][idx].contiguous(), [table["cam_model_host"][f] for f in chosen.tolist()])
        est = pose.estimate_poses(pk["matched_keypoints"][:S], pk["matched_xyzs"][:S], pk["counts"][:S], cams, seg_k=1,
                                  threshold=p["abs_pose_max_error"], trials=POSE_TRIALS, seed=p["seed"] + rnd)
        ni, cnt = est["num_inliers"][:S], pk["counts"][:S]
        ok = (est["success"][:S] != 0) & (ni >= p["abs_pose_min_num_inliers"]) & (ni.double() >= p["abs_pose_min_inlier_ratio"] * cnt.double())
        reg[idx] = ok.to(torch.uint8)
        tries[idx] += (~ok).to(torch.int32)
        fround[idx] = torch.where(ok, rnd, -1).to(torch.int32)
        qv_d, tv_d = qv_d.clone(), tv_d.clone()
        qv_d[idx] = torch.where(ok[:, None], est["qvec"][:S], qv_d[idx])
        tv_d[idx] = torch.where(ok[:, None], est["tvec"][:S], tv_d[idx])
        back = torch.cat([ok.int(), pk["cut"][:S]]).cpu().numpy()      # the acceptance: the round's second small read-back
        accepted = chosen[back[:S] != 0].tolist()
        if accepted:
            n_reg += len(accepted)
            m = grow(p["ba_iters"])
            qv_d, tv_d = m["qv"], m["tv"]
        rounds.append(line(m, chosen.tolist(), accepted, counts.tolist(), back[S:].tolist()))
    # ---- why a frame stayed out, from the last look at the correspondences
    n_corr, tried, reg_h = corr["n_corr"][:F].cpu().numpy(), tries[:F].cpu().numpy(), reg[:F].cpu().numpy().astype(bool)
    why = np.where(n_corr == 0, 0, np.where(n_corr < p["min_corr"], 1, np.where(tried >= p["max_reg_trials"], 2, 3)))
    unregistered = {int(f): REASONS[int(why[f])] for f in np.nonzero(~reg_h)[0].tolist()}
    # ---- the finish: one more triangulation at the final poses, the tables, one bundle adjustment
    t, out = _triangulate(table, v, adj, reg, qv_d, tv_d, p, n_reg, source=_verified(table, v, sc, pairs, matches, qv_d, tv_d, p))
    T, E = t["n_tracks"], t["n_entries"]
    tracks = {k: t[k].cpu().numpy() for k in ("trk_off", "trk_row", "trk_frame", "trk_kpt")}
    tri_h = {"accept": out["accept"][:T].cpu().numpy().astype(bool), "xyz": out["xyz"][:T].cpu().numpy(), "error": out["error"][:T].cpu().numpy(),
             "entry_keep": out["entry_keep"][:E].cpu().numpy().astype(bool)}
    model = tri._tables(frame_ids, table["frame_off_host"], [(tracks, tri_h)])[0]
    qv, tv = qv_d[:F].cpu().numpy(), tv_d[:F].cpu().numpy()
    frozen[reg_h] = 0
    frozen[a], frozen[b] = bundle.FROZEN_ALL, frozen_b
    ba = {k: x for k, x in p["bundle"].items() if k not in _BA_OWN}
    res = bundle.bundle_adjust(frames, cameras, (qv, tv), model, device, max_iters=p["final_ba_iters"], frozen=frozen, **ba)
    final_ba = res.pop("report")
    res.update(res_tail, registered=reg_h, frame_round=fround[:F].cpu().numpy(), seed_pair=seed,
               report={"success": True, "reason": None, "seed_frames": (a, b), "seed_relaxed": relaxed, "rounds": rounds,
                       "unregistered": unregistered, "final_ba": final_ba})
    return res
