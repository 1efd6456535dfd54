"""A map's 3D points on the device, from pairwise matches and known poses: the step between posed images and a ReferenceStore.

Reference: localization/triangulation.py (hloc's), which every dataset of the reference runs to get its SfM model.
  * import_matches / geometric_verification (triangulation.py:83-114, 131-202) with colmap_utils/geometry.py:10-17
    compute_epipolar_errors and colmap_utils/io.py find_pair / get_matches -> :func:`pair_matches`, :func:`unique_pairs`,
    :func:`verify_matches`.
  * run_triangulation (triangulation.py:205-223), which hands the verified matches to COLMAP's triangulator ->
    :func:`build_tracks` and :func:`triangulate_tracks`.
:func:`triangulate_map` runs all of it and returns what mapbuild.build_store_inputs and labelling.label_points take.  The
kernels are csrc/triangulate.hip; torch here is plumbing: uploads, the components' done flag, the table sizes
and one read-back of the results at the end.  profiles/triangulation_timing.md has the time of every stage.

Between verification and the tracks an optional stage 2b (:func:`support_matches`, ``min_support`` of :func:`triangulate_map`)
keeps a match only when ``min_support`` observations in third frames agree with it: a wrong match that lies on the epipolar line
passes verification by construction, and a single one joins two real tracks.  It is off by default (``min_support=0``);
profiles/triangulation_support.md has what it does to a simulated map and which value to use.  :func:`track_conflicts` counts,
per track, the frames seen twice: the sign that components are glued.

After stage 4 an optional number of further rounds (``split_rounds`` of :func:`triangulate_map`, :func:`split_edges`) takes apart
what stayed glued: sequential RANSAC over the match graph.  Every row has a state: TAKEN (a kept entry of an accepted track),
FREE (an entry of an accepted track that fell out as an outlier) or DEAD (everything else: rows of no track, and rows of a track
that was not accepted, which would come back identical).  A round keeps the edges of round 0 whose two ends are FREE, runs the
components, the tracks and stage 4 on them again, and its accepted tracks are further points.  A TAKEN or DEAD row never
returns, so every round with a track uses up two FREE rows at least; the rounds end at ``split_rounds``, or sooner when no edge
or no track is left.  It is off by default (``split_rounds=0``); profiles/triangulation_split.md has what each round recovers on
a simulated map, what it costs and which value to use.  It goes with stage 2b and does not replace it: one giant component
gives about one point per round.

The stages share one device-resident table of frames (:func:`frame_table`): the keypoints of all frames concatenated plus
frame_off, as StoreBase lays them out; a "row" is a keypoint's index in that table.

Where this differs from the reference, on purpose:
  * not COLMAP's triangulator.  A track is a connected component of the verified matches, not a transitive correspondence
    search from a seed observation; there is no Merge, Complete or Retriangulate and no bundle adjustment beyond a point-only
    refit (the poses are given and stay; localization/bundle.py refines them with the points afterwards).  The trial budget is fixed (every pair of a track's entries up to ``trials`` of them,
    else ``trials`` sampled pairs) instead of confidence-driven.  A component that wrong matches glued from two real points yields
    one of them at most: the hypothesis with most inliers wins and the other point's entries fall out as outliers.  Stage 2b
    removes most such matches before they join anything, where COLMAP accepts an observation only when it reprojects; a match
    that no third frame sees (a two-view track) cannot be confirmed and falls out with ``min_support`` >= 1, as it would later
    at the reference's own min_obs / obs_thresh of 3.  A component that stays glued after the filter yields one point per
    component per round: one with ``split_rounds=0``, and with further rounds the points that its outliers still support.
  * pixel offsets: verification reads the keypoints as stored (offset 0), triangulation adds 0.5, as in the reference
    (geometric_verification passes get_keypoints' array, import_features adds 0.5 for COLMAP).  The inconsistency is kept.
  * out-of-range indices: a match with a keypoint index outside its frame is dropped, where the reference would raise.
  * estimation_and_geometric_verification, the unknown-pose RANSAC of pycolmap.verify_matches, is localization/twoview.py
    (DESIGN.md 4.24): ``estimate_two_view_geometries=True`` of :func:`triangulate_map` puts it in the place of stage 2.  It is
    not COLMAP's estimator; that module's docstring lists the deviations.
  * the COLMAP database and model files are not written.
  * of a frame's several inliers in one track the one with the smallest error stays (the lowest row on a tie); COLMAP keeps
    whichever observation its search met first."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import formats

VERIFY_DEFAULTS = dict(max_error=4.0)      # geometric_verification's
TRI_DEFAULTS = dict(trials=128, seed=0, min_tri_angle=1.5, max_reproj_error=4.0)      # degrees and pixels: COLMAP's
DEFAULTS = {**VERIFY_DEFAULTS, **TRI_DEFAULTS}
SUPPORT_DEFAULTS = dict(min_support=0)      # stage 2b's confirming third views per match; 0: the stage does not run
SPLIT_DEFAULTS = dict(split_rounds=0)      # further rounds over the entries that fell out as outliers; 0: none
TWOVIEW_MAP_DEFAULTS = dict(estimate_two_view_geometries=False, twoview=None)      # stage 2 by twoview.py, and its parameters
CC_GROUP = 8      # rounds of the components enqueued per look at the done flag


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        from pram_amd._lib import PramHipError
        raise PramHipError("triangulation: expected a CUDA device (pram_amd has no CPU path)")
    return device


def _params(name: str, params: dict, defaults: dict) -> dict:
    unknown = set(params) - set(defaults)
    if unknown:
        raise TypeError(f"{name}: unknown parameters {sorted(unknown)}")
    return {**defaults, **params}


def _up(a: np.ndarray, device) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.shape[0] == 0:      # never an empty allocation behind a pointer
        a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
    return torch.from_numpy(a).to(device)


def _int_param(p: dict, name: str) -> dict:
    if int(p[name]) != p[name] or p[name] < 0:
        raise ValueError(f"{name}: an integer >= 0")
    return {**p, name: int(p[name])}


def _inlier_ratio(count: np.ndarray, match_off: np.ndarray) -> np.ndarray:
    n = np.diff(match_off)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, count / n, np.nan)


def _track_table(tracks: dict, keys, dev) -> dict:
    """A track table on the host (:func:`build_tracks`', or a caller's own) -> its arrays ``keys`` on the device and its sizes."""
    t = {k: _up(np.asarray(tracks[k], dtype=np.int32).reshape(-1), dev) for k in keys}
    t.update(n_tracks=np.asarray(tracks["trk_off"]).reshape(-1).shape[0] - 1, n_entries=int(np.asarray(tracks["trk_row"]).shape[0]))
    return t


# ------------------------------------------------------------------ host side: the match store and the pair list
def pair_matches(match_store, pairs: Sequence) -> list:
    """pairs: (name0, name1) -> per pair what colmap_utils/io.py get_matches returns, (matches int64 [m, 2], scores [m] or None):
    ``matches0`` read through formats.read_matches under find_pair's lookup order (a/b, then b/a reversed, then the two
    old-style names a_b and b_a reversed); a pair the store does not hold is a ValueError."""
    out = []
    for name0, name1 in pairs:
        for a, b, sep, reverse in ((name0, name1, "/", False), (name1, name0, "/", True), (name0, name1, "_", False), (name1, name0, "_", True)):
            if formats.names_to_pair(a, b, sep) in match_store:
                break
        else:
            raise ValueError(f"Could not find pair {(name0, name1)}... Maybe you matched with a different list of pairs? ")
        if sep == "/":
            m0, sc = formats.read_matches(match_store, a, b)
        else:      # the older flat name: the same two datasets, read the same way
            grp = match_store[formats.names_to_pair_old(a, b)]
            m0, sc = np.asarray(grp["matches0"]), (np.asarray(grp["matching_scores0"]) if "matching_scores0" in grp else None)
        idx = np.where(m0 != -1)[0]
        m = np.stack([idx, m0[idx].astype(np.int64)], -1)
        out.append((np.flip(m, -1) if reverse else m, None if sc is None else sc[idx]))
    return out


def unique_pairs(pairs) -> np.ndarray:
    """The positions of the pairs the reference processes: a pair whose (id0, id1) or (id1, id0) was already seen is skipped,
    the first occurrence wins (triangulation.py:102-108, 172-174)."""
    seen, keep = set(), []
    for i, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        if (a, b) in seen or (b, a) in seen:
            continue
        seen |= {(a, b), (b, a)}
        keep.append(i)
    return np.array(keep, dtype=np.int64)


# ------------------------------------------------------------------ the shared frame table
@torch.no_grad()
def frame_table(frames: Sequence[dict], cameras: Sequence, poses, device) -> dict:
    """frames: dicts with ``keypoints`` [n, 2] or [n, 3] (x, y[, score]) as ReferenceStore takes them; cameras: one
    (model_name, width, height, params) tuple per frame; poses: (qvecs [F, 4] (w, x, y, z), tvecs [F, 3]), cam_from_world
    -> the device-resident table every stage reads, with both normalisations of the keypoints (offset 0 and 0.5)."""
    from pram_amd.localization.pose import camera_table
    device = _device(device)
    F = len(frames)
    qv, tv = (np.asarray(x, dtype=np.float64) for x in poses)
    if len(cameras) != F or qv.shape != (F, 4) or tv.shape != (F, 3):
        raise ValueError(f"frame_table: {F} frames need {F} cameras, qvecs [{F}, 4] and tvecs [{F}, 3]")
    if not (np.isfinite(qv).all() and np.isfinite(tv).all() and (np.abs(qv).sum(1) > 0).all()):
        raise ValueError("frame_table: poses must be finite, quaternions not zero")
    ids, prm = camera_table(cameras)
    lens = [int(np.asarray(f["keypoints"]).shape[0]) for f in frames]
    if sum(lens) > 2 ** 30:
        raise ValueError("frame_table: more than 2^30 keypoints")
    frame_off = np.zeros(F + 1, dtype=np.int32)
    frame_off[1:] = np.cumsum(lens)
    kp = [np.asarray(f["keypoints"], dtype=np.float32).reshape(n, -1)[:, :2] for f, n in zip(frames, lens) if n]
    kp = np.concatenate(kp) if kp else np.zeros((0, 2), dtype=np.float32)
    n_rows = int(frame_off[-1])
    t = {"n_frames": F, "n_rows": n_rows, "frame_off_host": frame_off, "cam_model_host": ids.tolist(), "keypoints": _up(kp, device),
         "frame_off": _up(frame_off, device), "cam_model": _up(ids, device), "cam_params": _up(prm, device)}
    t["frames"] = ops.tri_frames(_up(qv, device), _up(tv, device), t["cam_model"], t["cam_params"], t["cam_model_host"])
    for key, off in (("norm0", 0.0), ("norm05", 0.5)):
        t[key] = ops.tri_normalize(t["keypoints"], t["frame_off"], t["cam_model"], t["cam_params"], t["cam_model_host"], n_rows, off)
    return t


def _match_csr(table: dict, pairs, matches: Sequence) -> tuple:
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(matches) != pairs.shape[0]:
        raise ValueError(f"{pairs.shape[0]} pairs, {len(matches)} match lists")
    if pairs.size and (pairs.min() < 0 or pairs.max() >= table["n_frames"]):
        raise ValueError("pairs: a frame index outside the table")
    use = unique_pairs(pairs)
    lists = [np.asarray(matches[i]).reshape(-1, 2) for i in use.tolist()]
    lens = np.array([m.shape[0] for m in lists], dtype=np.int64)
    if lens.sum() >= 2 ** 31:
        raise ValueError("matches: more than 2^31 - 1")
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    flat = np.concatenate(lists) if lists and lens.sum() else np.zeros((0, 2), dtype=np.int64)
    flat = np.where((flat >= -1) & (flat < 2 ** 31), flat, -1).astype(np.int32)      # whatever is out of range stays out of range
    return use, pairs[use].astype(np.int32), off, flat


# ------------------------------------------------------------------ the stages
@torch.no_grad()
def _verify(table: dict, pairs, matches, max_error: float) -> dict:
    use, pr, off, flat = _match_csr(table, pairs, matches)
    dev = table["keypoints"].device
    out = ops.tri_verify(table["norm0"], table["frame_off"], _up(pr, dev), _up(off, dev), _up(flat, dev), table["frames"], table["n_frames"],
                         len(use), flat.shape[0], max_error)
    out.update(pair_index=use, pairs=pr, match_off=off, n_matches=flat.shape[0])
    return out


def verify_matches(table: dict, pairs, matches: Sequence, **params) -> dict:
    """table: :func:`frame_table`; pairs [Pn, 2] frame indices; matches: per pair int [m, 2] (keypoint index in frame 0, in frame 1)
    -> on the host: ``pair_index`` (the positions of the pairs that were processed, :func:`unique_pairs`), and for each of them
    ``keep`` (bool mask over its matches), ``kept`` (the kept matches, original order) and ``inlier_ratio`` (nan for a pair
    without matches, which the reference leaves out of its statistics).  params: max_error."""
    p = _params("verify_matches", params, VERIFY_DEFAULTS)
    v = _verify(table, pairs, matches, p["max_error"])
    M, off = v["n_matches"], v["match_off"]
    keep, kept, count = v["keep"][:M].cpu().numpy().astype(bool), v["kept"][:M].cpu().numpy(), v["count"][:len(v["pair_index"])].cpu().numpy()
    return {"pair_index": v["pair_index"], "keep": [keep[a:b] for a, b in zip(off[:-1], off[1:])],
            "kept": [kept[a:a + c] for a, c in zip(off[:-1], count)], "inlier_ratio": _inlier_ratio(count, off)}


@torch.no_grad()
def _tracks(table: dict, edges: torch.Tensor, n_edges: int) -> dict:
    dev, n = table["keypoints"].device, table["n_rows"]
    label = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
    state = torch.empty(ops.TRI_CC_STATE_WORDS, device=dev, dtype=torch.int32)
    first = 0
    while True:      # every round at least halves the trees that still have an edge to another: ~log2(n_rows) rounds
        ops.tri_components(edges, n_edges, n, first, CC_GROUP, label, state)
        first += CC_GROUP
        if int(state[ops.TRI_CC_DONE].item()):
            break
    t = ops.tri_tracks(label, table["frame_off"], table["n_frames"], n)
    t["n_tracks"], t["n_entries"] = (int(x) for x in t["sizes"].cpu().tolist())
    t["label"] = label
    return t


def _edges(edges) -> np.ndarray:
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if e.shape[0] >= 2 ** 31:
        raise ValueError("edges: more than 2^31 - 1")
    return np.where((e >= -1) & (e < 2 ** 31), e, -1).astype(np.int32)


def build_tracks(table: dict, edges) -> dict:
    """edges: int [n, 2] rows of the table joined by a kept match (an edge with an end outside the table is ignored) -> on the
    host ``label`` int32 [n_rows] (every row's smallest connected row) and the tracks as CSR: ``trk_off`` int32 [T + 1],
    ``trk_label`` [T], ``trk_row`` / ``trk_frame`` / ``trk_kpt`` int32 [E].  A track is a component of two rows or more; tracks by
    ascending label, entries by ascending row: a function of the set of edges alone."""
    e = _edges(edges)
    t = _tracks(table, _up(e, table["keypoints"].device), e.shape[0])
    T, E = t["n_tracks"], t["n_entries"]
    return {"label": t["label"][:table["n_rows"]].cpu().numpy(), "trk_off": t["trk_off"][:T + 1].cpu().numpy(), "trk_label": t["trk_label"][:T].cpu().numpy(),
            **{k: t[k][:E].cpu().numpy() for k in ("trk_row", "trk_frame", "trk_kpt")}}


@torch.no_grad()
def _support(table: dict, edges: torch.Tensor, n_edges: int, p: dict) -> dict:
    a = ops.tri_adjacency(edges, n_edges, table["frame_off"], table["n_frames"], table["n_rows"])
    out = ops.tri_support(table["norm05"], table["keypoints"], table["frames"], table["cam_model"], table["cam_params"], edges, n_edges,
                          a["adj_off"], a["adj"], a["row_frame"], table["n_frames"], table["n_rows"],
                          min_tri_angle=float(np.deg2rad(p["min_tri_angle"])), max_reproj_error=p["max_reproj_error"], min_support=p["min_support"])
    out.update(a)
    return out


def adjacency(table: dict, edges) -> dict:
    """edges: int [n, 2] rows of the table (:func:`build_tracks`') -> on the host the rows' adjacency as stage 2b reads it:
    ``adj_off`` int32 [n_rows + 1], ``adj`` int32 [adj_off[-1]] (every row's neighbours ascending, one entry per edge, so a match
    given twice is there twice) and ``row_frame`` int32 [n_rows]."""
    e = _edges(edges)
    a = ops.tri_adjacency(_up(e, table["keypoints"].device), e.shape[0], table["frame_off"], table["n_frames"], table["n_rows"])
    off = a["adj_off"][:table["n_rows"] + 1].cpu().numpy()
    return {"adj_off": off, "adj": a["adj"][:int(off[-1])].cpu().numpy(), "row_frame": a["row_frame"][:table["n_rows"]].cpu().numpy()}


def support_matches(table: dict, edges, **params) -> dict:
    """Stage 2b on its own.  edges: int [n, 2] rows joined by a verified match -> on the host ``support`` int32 [n], the number of
    observations in third frames that confirm the match (a neighbour w of either end, in a frame of neither: of the three pairs of
    rays the one under the largest angle gives a point, and the two ends and w all reproject to it within max_reproj_error, that
    angle being min_tri_angle at least), ``keep`` (bool, support >= min_support) and ``edges`` int32 [n, 2], (-1, -1) where keep is
    false.  params: min_support (1 here), min_tri_angle (degrees), max_reproj_error (pixels)."""
    p = _int_param(_params("support_matches", params, dict(min_support=1, min_tri_angle=TRI_DEFAULTS["min_tri_angle"],
                                                           max_reproj_error=TRI_DEFAULTS["max_reproj_error"])), "min_support")
    e = _edges(edges)
    out = _support(table, _up(e, table["keypoints"].device), e.shape[0], p)
    sup = out["support"][:e.shape[0]].cpu().numpy()
    return {"support": sup, "keep": sup >= p["min_support"], "edges": out["edges"][:e.shape[0]].cpu().numpy()}


def track_conflicts(tracks: dict) -> np.ndarray:
    """tracks: :func:`build_tracks`' dict -> int64 [T]: per track the number of frames that hold more than one of its entries.  A
    point is seen once per frame, so a track with conflicts is two points or more that wrong matches glued together (numpy, on
    the host)."""
    off, frame = np.asarray(tracks["trk_off"], dtype=np.int64).reshape(-1), np.asarray(tracks["trk_frame"], dtype=np.int64).reshape(-1)
    T = off.shape[0] - 1
    if T <= 0 or frame.shape[0] == 0:
        return np.zeros(max(T, 0), dtype=np.int64)
    trk = np.repeat(np.arange(T), np.diff(off))
    _, first, count = np.unique(trk * (int(frame.max()) + 1) + frame, return_index=True, return_counts=True)
    return np.bincount(trk[first][count > 1], minlength=T).astype(np.int64)


@torch.no_grad()
def _triangulate(table: dict, t: dict, p: dict) -> dict:
    return ops.tri_triangulate(table["norm05"], table["keypoints"], table["frames"], table["cam_model"], table["cam_params"], t["trk_off"],
                               t["trk_label"], t["trk_row"], t["trk_frame"], t["n_tracks"], t["n_entries"], table["n_frames"], table["n_rows"],
                               trials=p["trials"], seed=p["seed"], min_tri_angle=float(np.deg2rad(p["min_tri_angle"])),
                               max_reproj_error=p["max_reproj_error"])


_TRI_KEYS = ("accept", "xyz", "error", "kept", "best")


def triangulate_tracks(table: dict, tracks: dict, **params) -> dict:
    """tracks: :func:`build_tracks`' dict (or the same arrays built otherwise; trk_kpt is not read) -> on the host, per track
    ``accept`` (bool), ``xyz`` float64 [T, 3], ``error`` (mean reprojection error of the kept entries, pixels), ``kept`` (their
    number), ``best`` (the winning hypothesis, -1: none), and per entry ``entry_keep`` (bool) and ``entry_error`` (pixels, -1 for
    an entry that is no inlier).  params: trials, seed, min_tri_angle (degrees), max_reproj_error (pixels)."""
    p = _params("triangulate_tracks", params, TRI_DEFAULTS)
    t = _track_table(tracks, ("trk_off", "trk_label", "trk_row", "trk_frame"), table["keypoints"].device)
    T, E = t["n_tracks"], t["n_entries"]
    out = _triangulate(table, t, p)
    res = {k: out[k][:T].cpu().numpy() for k in _TRI_KEYS}
    res["accept"] = res["accept"].astype(bool)
    res["entry_keep"], res["entry_error"] = out["entry_keep"][:E].cpu().numpy().astype(bool), out["entry_error"][:E].cpu().numpy()
    return res


@torch.no_grad()
def _split(table: dict, edges: torch.Tensor, n_edges: int, t: dict, out: dict, state) -> dict:
    return ops.tri_split(t["trk_off"], t["trk_row"], t["n_tracks"], t["n_entries"], out["accept"], out["entry_keep"], edges, n_edges,
                         table["n_rows"], state)


def split_edges(table: dict, edges, tracks: dict, tri: dict, state=None) -> dict:
    """The step between two rounds on its own.  edges: int [n, 2], the rows round 0's tracks were built from; tracks, tri: the last
    round's :func:`build_tracks` and :func:`triangulate_tracks`; state: uint8 [n_rows] from the round before, None before round 1
    (every row DEAD) -> on the host ``state`` uint8 [n_rows] (ops.TRI_ROW_FREE / TAKEN / DEAD) after marking the round's entries,
    ``edges`` int32 [n, 2], (-1, -1) where an end is not FREE, and ``n_live``, the number of edges that stay."""
    dev, n = table["keypoints"].device, table["n_rows"]
    e = _edges(edges)
    t = _track_table(tracks, ("trk_off", "trk_row"), dev)
    res = {"accept": _up(np.asarray(tri["accept"]).astype(np.int32).reshape(-1), dev),
           "entry_keep": _up(np.asarray(tri["entry_keep"]).astype(np.uint8).reshape(-1), dev)}
    if state is not None:
        state = np.asarray(state, dtype=np.uint8).reshape(-1)
        if state.shape[0] != n:
            raise ValueError(f"state: expected {n} rows, got {state.shape[0]}")
        state = _up(state, dev)
    out = _split(table, _up(e, dev), e.shape[0], t, res, state)
    return {"state": out["state"][:n].cpu().numpy(), "edges": out["edges"][:e.shape[0]].cpu().numpy(), "n_live": int(out["n_live"].item())}


@torch.no_grad()
def triangulate_map(frames: Sequence[dict], cameras: Sequence, poses, pairs, matches: Sequence, device, **params) -> dict:
    """frames, cameras, poses: :func:`frame_table`'s; pairs [Pn, 2] positions in ``frames`` and matches, per pair int [m, 2]:
    :func:`verify_matches`' (from :func:`pair_matches`, for instance) -> a dict:
      ``point_ids`` int64 [P], 1-based and ascending in track order over the accepted tracks; ``point3D_xyzs`` float64 [P, 3];
      ``track_error`` float64 [P]; ``tracks``: point id -> (image_ids, point2D_idxs), the dict mapbuild.track_tables takes (image
      ids are the frames' ``id``, by default their position); ``point3D_frame_ids``: point id -> image ids;
      ``frames``: per frame {``point3D_ids`` int64 [n], -1 where a keypoint has no point, ``xyzs`` float64 [n, 3]};
      ``pair_index`` and ``inlier_ratio`` as verify_matches gives them.
    With ``xyz = dict(zip(point_ids.tolist(), point3D_xyzs))``, labelling.label_points(tracks, xyz, k, device) and
    mapbuild.build_store_inputs(frames, tracks, landmarks, xyz, device) a ReferenceStore follows with no further tool.
    params: DEFAULTS and SUPPORT_DEFAULTS.  With ``min_support`` >= 1 the verified matches go through stage 2b
    (:func:`support_matches`) before the tracks, and the dict also holds ``support``: per processed pair an int32 array over its
    matches, -1 where verification had dropped the match.  The stages run back to back on the device; the results are read back
    once, at the end.
    params also SPLIT_DEFAULTS.  With ``split_rounds`` = R >= 1 up to R further rounds run over the entries that fell out of
    accepted tracks (the module docstring; :func:`split_edges` is the step between two rounds).  Round 0's points come first, so
    the first of them and their tracks are what ``split_rounds=0`` gives, bit for bit; then round 1's accepted tracks in track
    order, and so on.  The dict also holds ``point_round`` int32 [P] and ``split``: int64 arrays over the further rounds that were
    begun, ``live_edges`` (the edges between FREE rows; a round that finds none ends the rounds), ``tracks`` and ``points``.
    params also TWOVIEW_MAP_DEFAULTS.  With ``estimate_two_view_geometries=True`` (the reference's flag of the same name) stage 2
    is twoview.estimate_two_view's estimator instead of the test against the known poses: a pair's matches are kept when they
    agree with an essential matrix estimated from the matches themselves, so a pose that is off by more than ``max_error`` pixels
    no longer costs the pair its matches; the poses are still what stage 4 triangulates with.  ``twoview``: a dict of
    twoview.TWOVIEW_DEFAULTS' parameters (``max_error`` defaults to this call's).  The stages after it run on its edges as they
    are, and the dict also holds ``two_view``: ``E``, ``qvec``, ``tvec``, ``num_inliers``, ``num_front`` and ``success`` per
    processed pair, and ``keep``, per pair the mask over its matches."""
    p = _params("triangulate_map", params, {**DEFAULTS, **SUPPORT_DEFAULTS, **SPLIT_DEFAULTS, **TWOVIEW_MAP_DEFAULTS})
    p = _int_param(_int_param(p, "min_support"), "split_rounds")
    if p["estimate_two_view_geometries"]:
        from pram_amd.localization import twoview
        tv = twoview._twoview_params("triangulate_map: twoview", {"max_error": p["max_error"], **(p["twoview"] or {})})
    elif p["twoview"] is not None:
        raise ValueError("twoview: parameters of estimate_two_view_geometries=True")
    table = frame_table(frames, cameras, poses, device)
    v = twoview._estimate(table, pairs, matches, tv) if p["estimate_two_view_geometries"] else _verify(table, pairs, matches, p["max_error"])
    sup = _support(table, v["edges"], v["n_matches"], p) if p["min_support"] > 0 else None
    edges = v["edges"] if sup is None else sup["edges"]
    t = _tracks(table, edges, v["n_matches"])
    out = _triangulate(table, t, p)
    rounds, live, state = [(t, out)], [], None
    for _ in range(p["split_rounds"]):      # every round on the device; of a round only its sizes are read
        sp = _split(table, edges, v["n_matches"], t, out, state)
        state = sp["state"]
        live.append(int(sp["n_live"].item()))
        if live[-1] == 0:
            break
        t = _tracks(table, sp["edges"], v["n_matches"])
        if t["n_tracks"] == 0:
            break
        out = _triangulate(table, t, p)
        rounds.append((t, out))
    # ---- the one read-back
    Pn = len(v["pair_index"])
    host = []
    for t, out in rounds:
        T, E = t["n_tracks"], t["n_entries"]
        accept, xyz, err = out["accept"][:T].cpu().numpy().astype(bool), out["xyz"][:T].cpu().numpy(), out["error"][:T].cpu().numpy()
        keep = out["entry_keep"][:E].cpu().numpy().astype(bool)
        off, frame, kpt, row = (t[k].cpu().numpy() for k in ("trk_off", "trk_frame", "trk_kpt", "trk_row"))
        host.append(({"trk_off": off, "trk_row": row, "trk_frame": frame, "trk_kpt": kpt}, {"accept": accept, "xyz": xyz, "error": err, "entry_keep": keep}))
    frame_ids = np.array([f.get("id", i) for i, f in enumerate(frames)])
    res, point_round = _tables(frame_ids, table["frame_off_host"], host)
    if p["split_rounds"] > 0:
        K = len(live)      # the rounds begun; one that found no edge or no track has no tracks and no points
        n_tracks = [rounds[r][0]["n_tracks"] if r < len(rounds) else 0 for r in range(1, K + 1)]
        n_points = [int((point_round == r).sum()) for r in range(1, K + 1)]
        res.update(point_round=point_round, split={"live_edges": np.array(live, dtype=np.int64), "tracks": np.array(n_tracks, dtype=np.int64),
                                                   "points": np.array(n_points, dtype=np.int64)})
    res.update(pair_index=v["pair_index"], inlier_ratio=_inlier_ratio(v["count"][:Pn].cpu().numpy(), v["match_off"]))
    if p["estimate_two_view_geometries"]:
        keep = v["keep"][:v["n_matches"]].cpu().numpy().astype(bool)
        res["two_view"] = {**twoview._pair_results(v), "keep": [keep[a:b] for a, b in zip(v["match_off"][:-1], v["match_off"][1:])]}
    if sup is not None:
        M, m_off = v["n_matches"], v["match_off"]
        support = np.where(v["keep"][:M].cpu().numpy().astype(bool), sup["support"][:M].cpu().numpy(), -1).astype(np.int32)
        res["support"] = [support[a:b] for a, b in zip(m_off[:-1], m_off[1:])]
    return res


def map_tables(frame_ids, frame_off, tracks: dict, tri: dict, first_id: int = 1) -> dict:
    """The host's last step of :func:`triangulate_map`: the track table (:func:`build_tracks`) and the results
    (:func:`triangulate_tracks`) on the host -> point_ids, point3D_xyzs, track_error, tracks, point3D_frame_ids and frames as
    triangulate_map documents them.  The accepted tracks become points first_id, first_id + 1, ... in track order; a point's
    track holds its kept entries in ascending row."""
    return _tables(frame_ids, frame_off, [(tracks, tri)], first_id)[0]


def split_tables(frame_ids, frame_off, rounds: Sequence) -> dict:
    """:func:`map_tables` over several rounds.  rounds: per round (tracks, tri) on the host, round 0 first -> map_tables' dict with
    the rounds' points numbered one after the other, plus ``point_round`` int32 [P].  A row that a round kept is in no later
    round's table, so a keypoint has one point at most."""
    res, point_round = _tables(frame_ids, frame_off, rounds)
    return {**res, "point_round": point_round}


def _tables(frame_ids, frame_off, rounds: Sequence, first_id: int = 1) -> tuple:
    """The one builder behind :func:`map_tables` and :func:`split_tables`: a single pass over the rounds' accepted tracks fills the
    per-row point id and xyz -> (map_tables' dict, the points' round int32 [P])."""
    frame_ids, fo = np.asarray(frame_ids), np.asarray(frame_off)
    row_pid = np.full(int(fo[-1]), -1, dtype=np.int64)
    row_xyz = np.zeros((int(fo[-1]), 3), dtype=np.float64)
    out: Dict[int, tuple] = {}
    ids, xyzs, errs, nxt = [], [], [], first_id
    for tracks, tri in rounds:
        off, row, frame, kpt = (np.asarray(tracks[k]) for k in ("trk_off", "trk_row", "trk_frame", "trk_kpt"))
        accept, keep, xyz = np.asarray(tri["accept"]).astype(bool), np.asarray(tri["entry_keep"]).astype(bool), np.asarray(tri["xyz"])
        which = np.nonzero(accept)[0]
        ids.append(np.arange(nxt, nxt + which.shape[0], dtype=np.int64))
        xyzs.append(xyz[which].reshape(-1, 3))
        errs.append(np.asarray(tri["error"])[which])
        nxt += which.shape[0]
        for pid, ti in zip(ids[-1].tolist(), which.tolist()):
            e = np.arange(off[ti], off[ti + 1])[keep[off[ti]:off[ti + 1]]]
            out[pid] = (frame_ids[frame[e]], kpt[e].astype(np.int64))
            row_pid[row[e]], row_xyz[row[e]] = pid, xyz[ti]
    res = {"point_ids": np.concatenate(ids), "point3D_xyzs": np.concatenate(xyzs), "track_error": np.concatenate(errs), "tracks": out,
           "point3D_frame_ids": {pid: t[0] for pid, t in out.items()},
           "frames": [{"point3D_ids": row_pid[fo[f]:fo[f + 1]], "xyzs": row_xyz[fo[f]:fo[f + 1]]} for f in range(len(fo) - 1)]}
    return res, np.repeat(np.arange(len(ids)), [i.shape[0] for i in ids]).astype(np.int32)
