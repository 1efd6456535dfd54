"""Global bundle adjustment of a map on the device: the frames' poses refined together with the points, the step between
triangulation.triangulate_map on poses that drift and a map the localisation can solve against.

Reference: the reference's README sends custom data through "colmap or hloc to obtain the SfM results", that is, through
COLMAP's bundle adjustment; its own localization/triangulation.py runs pycolmap.triangulate_points, whose adjustment holds the
poses constant with refine_intrinsics=False.
  * :func:`bundle_adjust` on the dict triangulation.triangulate_map returns (or outliers.remove_statistical_outliers'
    restriction of it): poses and points together; with every frame frozen it is that points-only adjustment.
  * :func:`reprojection_errors`: the per-observation errors on their own.
The kernels are csrc/bundle.hip: Levenberg-Marquardt under the robust cost of the pose stage (per observation
s = |r|^2 / loss_scale^2, cost log1p(s), weight 1 / (1 + s)), the Schur complement's reduced camera system solved by matrix-free
conjugate gradients with the block-Jacobi preconditioner, the accept / reject decision and lam on the device, then COLMAP's point
filter.  torch here is plumbing: the observation tables (integers, built on the host), uploads, one look at the done word per
BA_GROUP iterations, one read-back at the end.  profiles/bundle_timing.md has the time of every stage.

Where this differs from COLMAP / Ceres, on purpose:
  * not Ceres: fixed budgets (``max_iters`` LM iterations of at most ``cg_iters`` CG iterations), pose.hip's damping
    H + lam diag(H) and its lam x 0.1 / x 10 rule instead of a trust region with a gain ratio;
  * the robust cost enters as IRLS weights, with no Triggs correction of the Gauss-Newton matrix;
  * intrinsics stay constant unless asked: ``refine_focal_length``, ``refine_principal_point`` and ``refine_extra_params``
    (COLMAP's names and meanings; "extra" is the distortion) refine the parameters of camera groups, the frames that share one
    physical camera (``camera_groups``), with the poses and the points.  Unlike COLMAP there are no priors on
    the parameters and no bogus-parameter filter beyond the test that a focal length stays finite and positive; as in COLMAP the
    principal point is off by default;
  * no Merge / Complete / Retriangulate between iterations: the tracks are the input's, the filter runs once, at the end.  Run
    triangulate_map again with the refined poses to get the tracks those poses support (INTEGRATION.md has the example);
  * the filter is COLMAP's FilterPoints3D as understood from its source: pycolmap is not installed and was never run beside
    this, so nothing here is pinned to it.  tests/bundle_ref.py is what the device equals, and that is checked on the CPU
    against a dense solve and scipy.
The gauge.  ``gauge='colmap'`` freezes all six parameters of the first frame that has observations and t_x of the second, which is
COLMAP's rule; ``gauge='none'`` freezes nothing (the damping keeps the system definite; the map may drift as a whole);
``frozen``: an int array [F] of six bits per frame (bit a freezes tangent parameter a: 0..2 rotation, 3..5 translation)
overrides the gauge.  A frozen parameter's step is exactly 0, and a frame that never moved returns its input pose bit for bit."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import triangulation as tri
from pram_amd.localization.outliers import restrict_model

# max_iters / cg_iters: profiles/bundle_timing.md has the iteration counts they were set from; lam0 is pose.hip's LM_LAMBDA0
BA_DEFAULTS = dict(max_iters=40, cg_iters=60, cg_tol=1e-2, ftol=1e-6, loss_scale=1.0, lam0=1e-3,
                   max_reproj_error=tri.TRI_DEFAULTS["max_reproj_error"], min_tri_angle=tri.TRI_DEFAULTS["min_tri_angle"], gauge="colmap",
                   frozen=None, refine_focal_length=False, refine_principal_point=False, refine_extra_params=False, camera_groups=None)
BA_GROUP = 4      # LM iterations enqueued per look at the done word
FROZEN_ALL = 63


def _ba_params(name: str, params: dict) -> dict:
    p = tri._params(name, params, BA_DEFAULTS)
    p = tri._int_param(tri._int_param(p, "max_iters"), "cg_iters")
    if p["max_iters"] > 4096 or p["cg_iters"] > 65536:
        raise ValueError("max_iters: at most 4096; cg_iters: at most 65536")
    for k in ("cg_tol", "ftol", "loss_scale", "lam0", "max_reproj_error", "min_tri_angle"):
        if not np.isfinite(float(p[k])):
            raise ValueError(f"{k}: must be finite")
    if not (0.0 < p["cg_tol"] < 1.0 and p["ftol"] >= 0.0 and p["loss_scale"] > 0.0 and p["lam0"] > 0.0 and p["max_reproj_error"] > 0.0
            and p["min_tri_angle"] >= 0.0):
        raise ValueError("needs 0 < cg_tol < 1, ftol >= 0, loss_scale > 0, lam0 > 0, max_reproj_error > 0, min_tri_angle >= 0")
    if p["gauge"] not in ("colmap", "none"):
        raise ValueError(f"gauge: 'colmap' or 'none', got {p['gauge']!r}")
    for k in REFINE_FLAGS:
        if not isinstance(p[k], (bool, np.bool_)):
            raise ValueError(f"{k}: True or False")
    return p


# ------------------------------------------------------------------ host side: the camera groups
REFINE_FLAGS = ("refine_focal_length", "refine_principal_point", "refine_extra_params")
# per model (COLMAP's parameter order): the indices of the focal lengths, of the principal point, of the extra parameters
PARAM_KINDS = {"SIMPLE_PINHOLE": ((0,), (1, 2), ()), "PINHOLE": ((0, 1), (2, 3), ()), "SIMPLE_RADIAL": ((0,), (1, 2), (3,)),
               "RADIAL": ((0,), (1, 2), (3, 4)), "OPENCV": ((0, 1), (2, 3), (4, 5, 6, 7))}
GROUP_FROZEN_ALL = 255


def _camera_key(cam) -> tuple:
    name, w, h, prm = cam
    return (str(name), int(w), int(h), np.asarray(prm, dtype=np.float64).tobytes())


def camera_groups(cameras: Sequence, groups=None) -> np.ndarray:
    """-> int32 [F], the group of every frame, numbered by first appearance.  ``groups`` None: frames whose camera tuples are equal
    (the same model, width and height, bit-equal parameters) share a group.  An array: int [F], frames with equal values share one
    camera; negative values, another shape or dtype, and a group whose frames differ in model, size or parameters raise."""
    F = len(cameras)
    keys = [_camera_key(c) for c in cameras]
    if groups is None:
        seen: dict = {}
        return np.array([seen.setdefault(k, len(seen)) for k in keys], dtype=np.int32).reshape(F)
    g = np.asarray(groups)
    if g.shape != (F,) or not np.issubdtype(g.dtype, np.integer):
        raise ValueError(f"camera_groups: an integer array [{F}]")
    if (g < 0).any():
        raise ValueError("camera_groups: values must not be negative")
    seen, first, out = {}, {}, np.zeros(F, dtype=np.int32)
    for f, v in enumerate(g.tolist()):
        q = seen.setdefault(v, len(seen))
        if first.setdefault(q, keys[f]) != keys[f]:
            raise ValueError(f"camera_groups: frame {f} differs from its group's camera in model, size or parameters")
        out[f] = q
    return out


def group_tables(cameras: Sequence, grp: np.ndarray, p: dict, masks=None) -> dict:
    """The groups' tables of pram_bac_begin on the host: ``frm_grp`` int32 [F], the CSR ``grp_off`` int32 [G + 1] / ``grp_frame``
    int32 [F] (ascending within a group), ``grp_params`` float64 [G, 8] (the model's own, zero padded), ``grp_mask`` int32 [G]
    (bit a freezes parameter a: what the three flags leave frozen, or-ed with ``masks`` [G] when given), and per group
    ``models`` (names) and ``first`` (its first frame)."""
    grp = np.asarray(grp, dtype=np.int32)
    G = int(grp.max()) + 1 if grp.shape[0] else 0
    order = np.argsort(grp, kind="stable")
    off = np.zeros(G + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(grp, minlength=G))
    first = order[off[:-1]]
    prm, mask, models = np.zeros((G, 8)), np.zeros(G, dtype=np.int32), []
    for q, f in enumerate(first.tolist()):
        name, _, _, x = cameras[f]
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        prm[q, :x.shape[0]] = x
        focal, pp, extra = PARAM_KINDS[str(name)]
        free = (focal if p["refine_focal_length"] else ()) + (pp if p["refine_principal_point"] else ()) + (extra if p["refine_extra_params"] else ())
        mask[q] = GROUP_FROZEN_ALL & ~sum(1 << a for a in free)
        models.append(str(name))
    if masks is not None:
        mask = mask | (np.asarray(masks, dtype=np.int32).reshape(G) & GROUP_FROZEN_ALL)
    return {"frm_grp": grp, "grp_off": off, "grp_frame": order.astype(np.int32), "grp_params": prm, "grp_mask": mask.astype(np.int32),
            "models": models, "first": first}


GROUP_KEYS = ("frm_grp", "grp_off", "grp_frame", "grp_params", "grp_mask")      # what goes to the device


# ------------------------------------------------------------------ host side: the observation tables and the gauge
def observation_tables(model: dict, frame_ids, frame_off) -> dict:
    """model: triangulate_map's dict; frame_ids: the frames' ``id`` in table order; frame_off int [F + 1] -> the integer tables of
    pram_ba_begin on the host: ``obs_row`` / ``obs_frame`` / ``obs_point`` int32 [O] in ascending row (frame-major), ``frm_off``
    int32 [F + 1], and the point-major CSR ``pt_off`` int32 [P + 1] / ``pt_obs`` int32 [O] (observation indices, ascending per
    point; numpy's stable sort).  A point is its position in ``point_ids``.  A track entry outside its frame, a frame id the table
    does not hold and a keypoint claimed by two points raise."""
    fo = np.asarray(frame_off, dtype=np.int64)
    F = fo.shape[0] - 1
    where = {fid: f for f, fid in enumerate(np.asarray(frame_ids).tolist())}
    if len(where) != F:
        raise ValueError("observation_tables: the frames' ids must be distinct")
    ids = np.asarray(model["point_ids"]).tolist()
    rows, pts = [], []
    for p, pid in enumerate(ids):
        img, kpt = model["tracks"][pid]
        img, kpt = np.asarray(img).reshape(-1).tolist(), np.asarray(kpt, dtype=np.int64).reshape(-1)
        try:
            f = np.array([where[i] for i in img], dtype=np.int64)
        except KeyError as e:
            raise ValueError(f"observation_tables: point {pid} is seen by frame id {e.args[0]}, which the frames do not hold") from None
        if f.shape != kpt.shape or (kpt < 0).any() or (kpt >= fo[f + 1] - fo[f]).any():
            raise ValueError(f"observation_tables: point {pid} names a keypoint outside its frame")
        rows.append(fo[f] + kpt)
        pts.append(np.full(f.shape[0], p, dtype=np.int64))
    row = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    pt = np.concatenate(pts) if pts else np.zeros(0, dtype=np.int64)
    order = np.argsort(row, kind="stable")
    row, pt = row[order], pt[order]
    if row.shape[0] > 1 and (np.diff(row) == 0).any():
        raise ValueError("observation_tables: a keypoint is in the tracks of two points (or twice in one)")
    if row.shape[0] > 2 ** 26:
        raise ValueError("observation_tables: more than 2^26 observations")
    frame = np.searchsorted(fo, row, side="right") - 1
    by_point = np.argsort(pt, kind="stable")
    pt_off = np.zeros(len(ids) + 1, dtype=np.int64)
    pt_off[1:] = np.cumsum(np.bincount(pt, minlength=len(ids)))
    entry_obs = np.empty(row.shape[0], dtype=np.int64)      # the observation of every track entry, the tracks one after the other
    entry_obs[order] = np.arange(row.shape[0])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return {"obs_row": i32(row), "obs_frame": i32(frame), "obs_point": i32(pt), "frm_off": i32(np.searchsorted(row, fo, side="left")),
            "pt_off": i32(pt_off), "pt_obs": i32(by_point), "entry_obs": entry_obs}


TABLE_KEYS = ("obs_row", "obs_frame", "obs_point", "frm_off", "pt_off", "pt_obs")      # what goes to the device


def gauge_mask(gauge: str, frozen, frm_off) -> np.ndarray:
    """-> int32 [F], six bits per frame.  ``frozen`` (an int array [F] with values 0 .. 63) wins; 'colmap': the first frame with
    observations fully, t_x (bit 3) of the second; 'none': zeros."""
    F = len(frm_off) - 1
    if frozen is not None:
        m = np.asarray(frozen)
        if m.shape != (F,) or not np.issubdtype(m.dtype, np.integer) or (m < 0).any() or (m > FROZEN_ALL).any():
            raise ValueError(f"frozen: an integer array [{F}] with values 0 .. 63")
        return m.astype(np.int32)
    m = np.zeros(F, dtype=np.int32)
    if gauge == "colmap":
        seen = np.nonzero(np.diff(np.asarray(frm_off)) > 0)[0]
        if seen.shape[0] > 0:
            m[seen[0]] = FROZEN_ALL
        if seen.shape[0] > 1:
            m[seen[1]] = 1 << 3
    return m


def _inputs(frames, poses, model) -> tuple:
    qv, tv = (np.ascontiguousarray(x, dtype=np.float64) for x in poses)
    ids = np.asarray(model["point_ids"])
    xyz = np.ascontiguousarray(model["point3D_xyzs"], dtype=np.float64).reshape(-1, 3)
    if xyz.shape[0] != ids.shape[0]:
        raise ValueError(f"model: {ids.shape[0]} point_ids, {xyz.shape[0]} point3D_xyzs")
    if not np.isfinite(xyz).all():
        raise ValueError("model: point3D_xyzs must be finite")
    frame_ids = np.array([f.get("id", i) for i, f in enumerate(frames)])
    return qv, tv, ids, xyz, frame_ids


@torch.no_grad()
def _run(table: dict, tabs: dict, xyz: np.ndarray, mask: np.ndarray, qv: np.ndarray, tv: np.ndarray, p: dict) -> tuple:
    """Everything on the device: the problem, the iterations in groups of BA_GROUP, the filter -> (problem, ops.ba_finish's dict)."""
    dev = table["keypoints"].device
    d = {k: tri._up(tabs[k], dev) for k in TABLE_KEYS}
    if p.get("groups") is not None:      # a refine flag is set: the entries that carry the groups' parameters
        gt = {k: tri._up(p["groups"][k], dev) for k in GROUP_KEYS}
        prob = ops.bac_begin(table["keypoints"], table["cam_model"], table["cam_model_host"], table["frames"], tri._up(xyz, dev), d["obs_row"],
                             d["obs_frame"], d["obs_point"], d["frm_off"], d["pt_off"], d["pt_obs"], tri._up(mask, dev), gt["frm_grp"], gt["grp_off"],
                             gt["grp_frame"], gt["grp_params"], gt["grp_mask"], xyz.shape[0], tabs["obs_row"].shape[0], table["n_rows"],
                             p["groups"]["grp_params"].shape[0], p["max_iters"], loss_scale=p["loss_scale"], lam0=p["lam0"], cg_tol=p["cg_tol"],
                             ftol=p["ftol"])
        state = prob["views"]["state_i32"]
        for _ in range(0, p["max_iters"], BA_GROUP):
            ops.bac_iterate(prob, BA_GROUP, p["cg_iters"])
            if int(state[ops.BA_SI_DONE].item()):
                break
        out = ops.bac_finish(prob, tri._up(qv, dev), tri._up(tv, dev), max_reproj_error=p["max_reproj_error"],
                             min_tri_angle=float(np.deg2rad(p["min_tri_angle"])))
        return prob, out
    prob = ops.ba_begin(table["keypoints"], table["cam_model"], table["cam_params"], table["cam_model_host"], table["frames"], tri._up(xyz, dev),
                        d["obs_row"], d["obs_frame"], d["obs_point"], d["frm_off"], d["pt_off"], d["pt_obs"], tri._up(mask, dev), xyz.shape[0],
                        tabs["obs_row"].shape[0], table["n_rows"], p["max_iters"], loss_scale=p["loss_scale"], lam0=p["lam0"], cg_tol=p["cg_tol"],
                        ftol=p["ftol"])
    state = prob["views"]["state_i32"]
    for _ in range(0, p["max_iters"], BA_GROUP):      # the done word ends the run; the launches behind it return at once
        ops.ba_iterate(prob, BA_GROUP, p["cg_iters"])
        if int(state[ops.BA_SI_DONE].item()):
            break
    out = ops.ba_finish(prob, tri._up(qv, dev), tri._up(tv, dev), max_reproj_error=p["max_reproj_error"],
                        min_tri_angle=float(np.deg2rad(p["min_tri_angle"])))
    return prob, out


def _report(prob: dict, out: dict, n_obs: int) -> dict:
    sd, si = prob["views"]["state_f64"].cpu().numpy(), prob["views"]["state_i32"].cpu().numpy()
    K, n = prob["max_iters"], int(si[ops.BA_SI_LM_ITER])
    counts, pt_keep = out["counts"].cpu().numpy(), out["pt_keep"].cpu().numpy()
    reason = ops.BA_REASONS.get(int(si[ops.BA_SI_REASON]), "unknown")
    if reason == "tables":
        raise ops._lib.PramHipError("bundle_adjust: the observation tables failed the check on the device")
    return {"initial_cost": float(sd[ops.BA_SD_COST0]), "final_cost": float(sd[ops.BA_SD_COST]), "lm_iterations": n,
            "lm_accepted": int(si[ops.BA_SI_ACCEPTED]), "cg_iterations": si[ops.BA_STATE_I32:ops.BA_STATE_I32 + n].astype(np.int64),
            "accepted": si[ops.BA_STATE_I32 + K:ops.BA_STATE_I32 + K + n].astype(bool), "cg_breakdowns": int(si[ops.BA_SI_CG_FAIL]),
            "lam": float(sd[ops.BA_SD_LAM]), "observations": n_obs, "zero_weight_observations": int(counts[0]),
            "filtered_observations": int(counts[1]), "filtered_points": int((pt_keep == 0).sum()),
            "unsolvable_points": int((prob["views"]["point_ok"].cpu().numpy() == 0).sum()), "termination": reason}


def clean_model(model: dict, tabs: dict, frame_off, xyz: np.ndarray, pt_keep: np.ndarray, pt_error: np.ndarray, obs_keep: np.ndarray) -> dict:
    """The host's last step of :func:`bundle_adjust` (numpy): the input model, :func:`observation_tables`, the refined points and
    the filter's masks -> the model with the filtered points removed as outliers.restrict_model removes them, the filtered
    observations taken out of the kept points' tracks, and ``point3D_xyzs`` / ``track_error`` / the frames' ``xyzs`` set from the
    refined points."""
    fo = np.asarray(frame_off, dtype=np.int64)
    keep, obs_keep = np.asarray(pt_keep).astype(bool), np.asarray(obs_keep).astype(bool)
    ids = np.asarray(model["point_ids"])
    refined = dict(model)
    refined["point3D_xyzs"], refined["track_error"] = np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(pt_error, dtype=np.float64)
    out = restrict_model(refined, keep)
    tracks = {}
    for p in np.nonzero(keep)[0].tolist():
        pid = ids[p].item()
        img, kpt = (np.asarray(a).reshape(-1) for a in model["tracks"][pid])
        m = obs_keep[tabs["entry_obs"][tabs["pt_off"][p]:tabs["pt_off"][p + 1]]]
        tracks[pid] = (img[m], kpt[m])
    out["tracks"], out["point3D_frame_ids"] = tracks, {pid: t[0] for pid, t in tracks.items()}
    if "frames" in model:
        row, pt = tabs["obs_row"].astype(np.int64), tabs["obs_point"]
        stays = obs_keep & keep[pt]
        row_pid = np.full(int(fo[-1]), -1, dtype=np.int64)
        row_xyz = np.zeros((int(fo[-1]), 3), dtype=np.float64)
        row_pid[row[stays]], row_xyz[row[stays]] = ids[pt[stays]], refined["point3D_xyzs"][pt[stays]]
        out["frames"] = [{**f, "point3D_ids": row_pid[fo[i]:fo[i + 1]], "xyzs": row_xyz[fo[i]:fo[i + 1]]} for i, f in enumerate(model["frames"])]
    return out


def _solve(frames: Sequence[dict], cameras: Sequence, poses, model: dict, device, p: dict) -> tuple:
    qv, tv, ids, xyz, frame_ids = _inputs(frames, poses, model)
    table = tri.frame_table(frames, cameras, (qv, tv), device)
    tabs = observation_tables(model, frame_ids, table["frame_off_host"])
    mask = gauge_mask(p["gauge"], p["frozen"], tabs["frm_off"])
    table["camera_groups"] = camera_groups(cameras, p["camera_groups"])
    table["groups"] = group_tables(cameras, table["camera_groups"], p) if any(p[k] for k in REFINE_FLAGS) else None
    if tabs["obs_row"].shape[0] == 0:
        return table, tabs, qv, tv, xyz, None, None
    prob, out = _run(table, tabs, xyz, mask, qv, tv, {**p, "groups": table["groups"]})
    return table, tabs, qv, tv, xyz, prob, out


def _intrinsics(cameras: Sequence, table: dict, tabs: dict, refined) -> tuple:
    """-> (the cameras of the result, report['intrinsics']): per group its model, frame and observation counts, the mask used and
    the parameters before and after.  refined: float64 [G, 8] or None (nothing was refined: every frame gets its input tuple)."""
    gt = table["groups"]
    if gt is None:
        return list(cameras), []
    n_obs = np.diff(np.asarray(tabs["frm_off"], dtype=np.int64))
    cams, rows = list(cameras), []
    for q, name in enumerate(gt["models"]):
        fr = gt["grp_frame"][gt["grp_off"][q]:gt["grp_off"][q + 1]]
        n = ops.CAMERA_NUM_PARAMS[ops.CAMERA_MODELS[name]]
        obs = int(n_obs[fr].sum())
        used = GROUP_FROZEN_ALL if obs == 0 else int(gt["grp_mask"][q]) | (GROUP_FROZEN_ALL & ~((1 << n) - 1))
        before = gt["grp_params"][q, :n].copy()
        after = before.copy() if refined is None else np.asarray(refined[q, :n], dtype=np.float64).copy()
        rows.append({"model": name, "frames": int(fr.shape[0]), "observations": obs, "mask": used, "params_before": before, "params_after": after})
        if used != GROUP_FROZEN_ALL and not np.array_equal(before, after):
            for f in fr.tolist():
                cams[f] = (cameras[f][0], cameras[f][1], cameras[f][2], after.copy())
    return cams, rows


def bundle_adjust(frames: Sequence[dict], cameras: Sequence, poses, model: dict, device, **params) -> dict:
    """frames, cameras, poses: triangulation.frame_table's (the poses cam_from_world: qvecs [F, 4] (w, x, y, z), tvecs [F, 3]);
    model: the dict triangulation.triangulate_map returns, or outliers.remove_statistical_outliers' restriction of it -> a dict of
    the same shape: ``point_ids`` (preserved; the filtered points are gone), ``point3D_xyzs`` (refined), ``track_error``
    (recomputed: the mean reprojection error of a point's kept observations), ``tracks`` / ``point3D_frame_ids`` / the frames'
    ``point3D_ids`` and ``xyzs`` without the filtered points and observations; every other key passes through.  Added: ``qvecs``
    float64 [F, 4] and ``tvecs`` [F, 3], the refined poses, ``removed_ids``, and ``report``: ``initial_cost``, ``final_cost``,
    ``lm_iterations``, ``lm_accepted``, ``accepted`` (bool per iteration), ``cg_iterations`` (per iteration), ``cg_breakdowns``,
    ``lam``, ``observations``, ``zero_weight_observations``, ``filtered_observations``, ``filtered_points``, ``unsolvable_points``
    and ``termination`` ('max_iters', 'ftol', or 'empty' for a model without observations).  params: BA_DEFAULTS (the module
    docstring has the gauge).  ``refine_focal_length`` / ``refine_principal_point`` / ``refine_extra_params`` (booleans, default
    False) refine the intrinsics of the camera groups; ``camera_groups``: None (frames whose camera tuples are equal share a group,
    :func:`camera_groups`) or an int array [F].  With all three False the adjustment is the one with constant intrinsics, bit for
    bit.  The result also has ``cameras`` (one (model_name, width, height, params) tuple per frame, refined; a frame of a group that
    was not refined gets its input tuple back), ``camera_groups`` (the array used) and ``report['intrinsics']`` (per group
    ``model``, ``frames``, ``observations``, ``mask``, ``params_before``, ``params_after``; empty when nothing was asked).  A group
    without observations is frozen.  Give ``result['cameras']`` to whatever reads the map afterwards (frame_table,
    DatabaseStore.from_triangulation).  With ``max_iters=0`` the poses and the points come back bit for bit and only the filter runs.
    Everything is read back once, at the end.  The input is not modified."""
    p = _ba_params("bundle_adjust", params)
    table, tabs, qv, tv, xyz, prob, out = _solve(frames, cameras, poses, model, device, p)
    if prob is None:
        report = {"initial_cost": 0.0, "final_cost": 0.0, "lm_iterations": 0, "lm_accepted": 0, "accepted": np.zeros(0, dtype=bool),
                  "cg_iterations": np.zeros(0, dtype=np.int64), "cg_breakdowns": 0, "lam": float(p["lam0"]), "observations": 0,
                  "zero_weight_observations": 0, "filtered_observations": 0, "filtered_points": int(xyz.shape[0]), "unsolvable_points": 0,
                  "termination": "empty"}
        res = clean_model(model, tabs, table["frame_off_host"], xyz, np.zeros(xyz.shape[0], dtype=bool), np.zeros(xyz.shape[0]), np.zeros(0, dtype=bool))
        cams, report["intrinsics"] = _intrinsics(cameras, table, tabs, None)
        res.update(qvecs=qv.copy(), tvecs=tv.copy(), removed_ids=np.asarray(model["point_ids"]), report=report, cameras=cams,
                   camera_groups=table["camera_groups"])
        return res
    # ---- the one read-back
    report = _report(prob, out, tabs["obs_row"].shape[0])
    host = {k: out[k].cpu().numpy() for k in ("qvec", "tvec", "xyz", "obs_keep", "pt_keep", "pt_error")}
    res = clean_model(model, tabs, table["frame_off_host"], host["xyz"], host["pt_keep"], host["pt_error"], host["obs_keep"])
    cams, report["intrinsics"] = _intrinsics(cameras, table, tabs, out["grp_params"].cpu().numpy() if "grp_params" in out else None)
    res.update(qvecs=host["qvec"], tvecs=host["tvec"], removed_ids=np.asarray(model["point_ids"])[host["pt_keep"] == 0], report=report,
               cameras=cams, camera_groups=table["camera_groups"])
    return res


def reprojection_errors(frames: Sequence[dict], cameras: Sequence, poses, model: dict, device) -> dict:
    """The model's observations through the full camera model at the given poses -> on the host ``error`` float64 [O] (pixels,
    against keypoint + 0.5), ``front`` bool [O] (positive depth), and the observations themselves: ``frame`` (position in
    ``frames``), ``keypoint`` and ``point_id``, in ascending (frame, keypoint)."""
    p = _ba_params("reprojection_errors", {"max_iters": 0, "max_reproj_error": np.finfo(np.float64).max ** 0.5})
    table, tabs, _, _, _, prob, out = _solve(frames, cameras, poses, model, device, p)
    fo = np.asarray(table["frame_off_host"], dtype=np.int64)
    f = tabs["obs_frame"].astype(np.int64)
    res = {"frame": f, "keypoint": tabs["obs_row"] - fo[f], "point_id": np.asarray(model["point_ids"])[tabs["obs_point"]]}
    if prob is None:
        return {**res, "error": np.zeros(0), "front": np.zeros(0, dtype=bool)}
    _report(prob, out, 0)      # raises when the tables failed the device's check
    return {**res, "error": out["obs_error"].cpu().numpy(), "front": out["obs_keep"].cpu().numpy().astype(bool)}

