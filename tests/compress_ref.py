"""numpy restatement of the reference's map compression (RecMap.compress_map_by_projection_v2, recognition/recmap.py:668-922) and
of RefFrame.associate_keypoints_with_point3Ds (localization/refframe.py:99-147) as pram_amd.localization.compress runs them on the
device, and the scene the tests share.

Every projection is written with separate multiplies and adds in the kernel's order (csrc/compress.hip: project), so the device's
float64 numbers are reproduced bit for bit; the reference's own come from BLAS products and may differ in the last bits, which the
scene's margins (asserted by tests/tools/gen_compress_pinned.py from the traces kept here) keep from deciding anything.
"""
from __future__ import annotations

import numpy as np

SEED = 20240323
F, FRAME_ID0, N_POINTS = 14, 200, 1200
WIDTH, HEIGHT, INTRINSICS = 640, 480, (520.0, 515.0, 320.0, 240.0)
ROW_TILE, KPT_TILE = 256, 256      # include/pram_hip.h: PRAM_COMPRESS_ROW_TILE, PRAM_COMPRESS_KPT_TILE
# rows per frame: several tiles, both sides of one tile, no multiple of 64, under 64
ROWS = [600, 520, 300, 257, 256, 255, 100, 40, 400, 350, 280, 200, 150, 320]
FRAME_A, FRAME_LOSER, FRAME_TWICE = 0, 7, 2
# landmark -> frames; with vrf_frames = 1 the reference frames are 0, 8, 2, 1: frame 0 is named twice, frame 8 is a candidate of 0
SEG_REF = {0: [0, 3], 1: [8, 1], 2: [0, 5], 3: [2, 9], 4: [1, 4]}
RADIUS = 20.0
CONFIGS = {"c5": dict(covisible_frames=5, nkpts=-1), "c30": dict(covisible_frames=30, nkpts=-1), "c30n100": dict(covisible_frames=30, nkpts=100)}
UNKNOWN_ID0 = 70000


# ------------------------------------------------------------------------------------------------ projections
def rotation(q):
    qw, qx, qy, qz = (float(x) for x in q)
    return (1.0 - 2.0 * qy * qy - 2.0 * qz * qz, 2.0 * qx * qy - 2.0 * qw * qz, 2.0 * qz * qx + 2.0 * qw * qy,
            2.0 * qx * qy + 2.0 * qw * qz, 1.0 - 2.0 * qx * qx - 2.0 * qz * qz, 2.0 * qy * qz - 2.0 * qw * qx,
            2.0 * qz * qx - 2.0 * qw * qy, 2.0 * qy * qz + 2.0 * qw * qx, 1.0 - 2.0 * qx * qx - 2.0 * qy * qy)


def project(cam, xyz):
    """cam: one row (qvec, tvec, fx, fy, cx, cy, width, height); xyz [n, 3] -> (u, v, Z), each [n]."""
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = rotation(cam[0:4])
    tx, ty, tz, fx, fy, cx, cy = (float(x) for x in cam[4:11])
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    X = r00 * x + r01 * y + r02 * z + tx
    Y = r10 * x + r11 * y + r12 * z + ty
    Z = r20 * x + r21 * y + r22 * z + tz
    with np.errstate(divide="ignore", invalid="ignore"):
        return (fx * X + cx * Z) / Z, (fy * Y + cy * Z) / Z, Z


# ------------------------------------------------------------------------------------------------ stage 1
def covisible_lists(frame_off, row_ids, point_frames, frames, n):
    """The store's rule for the frames asked for: per valid row every entry of its point's list counts once (the frame itself
    included); count descending, frame index ascending, cut at n.  -> {frame: (frames, counts, all counts before the cut)}."""
    out = {}
    for f in frames:
        cnt = {}
        for pid in row_ids[frame_off[f]:frame_off[f + 1]].tolist():
            if pid != -1 and pid in point_frames:
                for g in point_frames[pid]:
                    cnt[g] = cnt.get(g, 0) + 1
        order = sorted(cnt, key=lambda g: (-cnt[g], g))
        out[f] = (order[:n], [cnt[g] for g in order[:n]], sorted(cnt.values()))
    return out


def min_distance(u, w, kp):
    """recmap.py:732-735: the smallest sqrt(dx * dx + dy * dy) from every (u, w) to the keypoints kp [m, 2]."""
    dx, dy = u[:, None] - kp[None, :, 0], w[:, None] - kp[None, :, 1]
    return np.sqrt(dx * dx + dy * dy).min(axis=1)


def select(frame_off, row_ids, pt_ids, pt_xyz, xys, cams, covis, vrf, radius, skip_decided=False, min_dist=min_distance):
    """recmap.py:771-828 on store frame indices.  covis: frame -> candidates in order; vrf: the reference frames in order.
    -> (retained frames in order, kept flag per row, trace).  The trace holds the smallest margins of every decision.
    skip_decided: a row some chain frame already discarded is not measured again (the same result for less work: the timing tool's
    choice); min_dist: the distance step, for a caller with a faster one."""
    pos = np.clip(np.searchsorted(pt_ids, row_ids), 0, max(len(pt_ids) - 1, 0))
    valid = (row_ids != -1) & (pt_ids[pos] == row_ids) if len(pt_ids) else np.zeros(len(row_ids), dtype=bool)
    row_pt = np.where(valid, pos, -1)
    kept = np.zeros(len(row_ids), dtype=bool)
    retained = []
    trace = {"radius_margin": np.inf, "border_margin": np.inf, "depth_margin": np.inf, "lost_all": [], "overwritten": [], "appended": 0,
             "tested": 0, "outside": 0, "behind": 0, "empty_chain_frame": 0}
    for v in vrf:
        a, b = frame_off[v], frame_off[v + 1]
        if v in retained and int(kept[a:b].sum()) < int(valid[a:b].sum()):
            trace["overwritten"].append(v)
        kept[a:b] = valid[a:b]
        if v not in retained:
            retained.append(v)
        chain = [v]
        for c in covis[v]:
            if c == v:
                continue
            if c in retained:
                chain.append(c)
                trace["appended"] += 1
                continue
            rows = np.arange(frame_off[c], frame_off[c + 1])[valid[frame_off[c]:frame_off[c + 1]]]
            if len(rows) == 0:
                continue
            xyz = pt_xyz[row_pt[rows]]
            alive = np.ones(len(rows), dtype=bool)
            trace["tested"] += 1
            for k in chain:
                u, w, Z = project(cams[k], xyz)
                width, height = cams[k][11], cams[k][12]
                inside = (u >= 0) & (u < width) & (w >= 0) & (w < height)
                front = Z > 0
                trace["outside"] += int((~inside).sum())
                trace["behind"] += int((~front).sum())
                with np.errstate(invalid="ignore"):
                    trace["border_margin"] = min(trace["border_margin"], float(np.nanmin(np.abs(np.stack([u, u - width, w, w - height])))))
                trace["depth_margin"] = min(trace["depth_margin"], float(np.abs(Z).min()))
                kp = xys[frame_off[k]:frame_off[k + 1]][kept[frame_off[k]:frame_off[k + 1]]]
                if len(kp) == 0:
                    trace["empty_chain_frame"] += 1
                    continue
                consider = inside & front
                need = consider & alive if skip_decided else np.ones(len(rows), dtype=bool)      # the reference measures every row
                dmin = np.full(len(rows), np.inf)
                if need.any():
                    dmin[need] = min_dist(u[need], w[need], kp)
                if (consider & need).any():
                    trace["radius_margin"] = min(trace["radius_margin"], float(np.abs(dmin[consider & need] - radius).min()))
                with np.errstate(invalid="ignore"):
                    alive &= ~(consider & (dmin <= radius))
            if not alive.any():
                trace["lost_all"].append((v, c))
                continue
            kept[rows[alive]] = True
            retained.append(c)
            chain.append(c)
    return retained, kept, trace


# ------------------------------------------------------------------------------------------------ stage 2
def sparsify(cam, xyz, scores, radius):
    """sparsify_by_grid (recmap.py:670-693) on the projections with the frame's own pose -> (the winners' positions in the order in
    which their cells first appear, the smallest distance of a u or v from a multiple of the radius)."""
    u, v, _ = project(cam, xyz)
    nw = int(np.ceil(cam[11] / radius))
    grid, margin = {}, np.inf
    for ip in range(len(u)):
        if not (np.isfinite(u[ip]) and np.isfinite(v[ip])):
            continue
        for t in (u[ip], v[ip]):
            margin = min(margin, abs(t - radius * np.round(t / radius)))
        iw, ih = int(np.rint(u[ip] // radius)), int(np.rint(v[ip] // radius))
        idx = ih * nw + iw
        if idx in grid:
            if scores[ip] <= grid[idx][0]:
                continue
            grid[idx] = (scores[ip], ip)      # a dict keeps the key's first place
        else:
            grid[idx] = (scores[ip], ip)
    return np.array([grid[k][1] for k in grid], dtype=np.int64), margin


# ------------------------------------------------------------------------------------------------ all stages
def compress(s: dict, covisible_frames: int, nkpts: int, radius: float = RADIUS) -> dict:
    """The three outputs on scene s: ``frames`` (store frame indices, retained order), ``lists`` (frame -> point ids) and
    ``point_frames`` (point id -> frames, in order of first appearance), with the trace."""
    vrf = vrf_order(s["seg_ref"], 1)
    lists = covisible_lists(s["frame_off"], s["point3D_ids"], s["point_frames"], sorted(set(vrf)), covisible_frames)
    retained, kept, trace = select(s["frame_off"], s["point3D_ids"], s["pt_ids"], s["pt_xyz"], s["xys"], s["cams"],
                                   {f: lists[f][0] for f in lists}, vrf, radius)
    trace["covis_counts"] = {f: lists[f][2] for f in lists}
    trace["cut"] = {f: len(lists[f][2]) > covisible_frames for f in lists}
    trace["cell_margin"], trace["sparsified"] = np.inf, []
    out, point_frames = {}, {}
    for f in retained:
        a, b = s["frame_off"][f], s["frame_off"][f + 1]
        ids = s["point3D_ids"][a:b][kept[a:b]]
        if nkpts > 0 and len(ids) > nkpts:
            at = np.searchsorted(s["pt_ids"], ids)
            win, margin = sparsify(s["cams"][f], s["pt_xyz"][at], s["pt_obs"][at], radius)
            trace["cell_margin"] = min(trace["cell_margin"], margin)
            trace["sparsified"].append(f)
            ids = ids[win]
        out[f] = ids
        for p in ids.tolist():
            point_frames.setdefault(p, []).append(f)
    return {"frames": retained, "lists": out, "point_frames": point_frames, "trace": trace}


def vrf_order(seg_ref, vrf_frames=1):
    """recmap.py:749-761."""
    out = []
    for v in seg_ref.values():
        for f in list(v)[:vrf_frames]:
            if f not in out:
                out.append(f)
    return out


def frame_rows(s: dict, f: int, ids) -> dict:
    """associate_keypoints_with_point3Ds for frame f listing the point ids ``ids`` (all in the table): keypoints [n, 3], xyzs."""
    at = np.searchsorted(s["pt_ids"], np.asarray(ids, dtype=np.int64))
    xyz = s["pt_xyz"][at]
    u, v, _ = project(s["cams"][f], xyz)
    score = 1 / np.clip(s["pt_err"][at] * 5, a_min=1.0, a_max=20.0)
    return {"keypoints": np.stack([u, v, score], axis=1), "xyzs": xyz, "point3D_ids": np.asarray(ids, dtype=np.int64),
            "keypoint_segs": s["pt_sid"][at]}


# ------------------------------------------------------------------------------------------------ the scene
_scene_cache = {}


def scene(seed: int = SEED) -> dict:
    """The shared scene (cached; treat as read-only): F frames on one camera, ROWS[f] rows each, sharing about N_POINTS points."""
    if seed in _scene_cache:
        return _scene_cache[seed]
    rng = np.random.default_rng(seed)
    # a world wider than one image: a frame sees a part of it, so that many rows of a candidate fall outside a chain frame
    xyz_all = np.stack([rng.uniform(-6.0, 6.0, N_POINTS), rng.uniform(-4.0, 4.0, N_POINTS), rng.uniform(5.5, 8.5, N_POINTS)], axis=1)
    cams = np.zeros((F, 13))
    for f in range(F):
        q = np.array([1.0, *(0.03 * rng.standard_normal(3))])
        cams[f, 0:4], cams[f, 4:7] = q / np.linalg.norm(q), [rng.uniform(-3.5, 3.5), rng.uniform(-2.0, 2.0), rng.uniform(-0.5, 0.5)]
        cams[f, 7:11], cams[f, 11], cams[f, 12] = INTRINSICS, WIDTH, HEIGHT
    cams[FRAME_LOSER, 4:7] = cams[FRAME_A, 4:7] + [0.3, -0.2, 0.1]      # the loser stands beside frame A
    visible = []
    for f in range(F):
        u, v, Z = project(cams[f], xyz_all)
        visible.append(np.nonzero((u > 2) & (u < WIDTH - 2) & (v > 2) & (v < HEIGHT - 2) & (Z > 0))[0])
    # the points each frame observes: drawn around a centre of its own, so that the frames share different numbers of points
    observed = [None] * F
    n_bad = [max(3, n // 20) for n in ROWS]      # rows with id -1 and, two of them, ids the table lacks
    for f in range(F):
        if f == FRAME_LOSER:
            continue
        centre = -cams[f, 4:6] + np.array([rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0)])
        w = np.exp(-((xyz_all[visible[f], :2] - centre) ** 2).sum(1) / 6.0)
        n = min(ROWS[f] - n_bad[f], len(visible[f]))
        observed[f] = rng.choice(visible[f], size=n, replace=False, p=w / w.sum())
    # the loser sees only points that frame A sees too, each of them inside A's image: A's keypoints cover every one of its rows
    pool = np.intersect1d(observed[FRAME_A], visible[FRAME_LOSER])
    observed[FRAME_LOSER] = rng.choice(pool, size=ROWS[FRAME_LOSER] - n_bad[FRAME_LOSER], replace=False)
    frame_off = np.zeros(F + 1, dtype=np.int32)
    frame_off[1:] = np.cumsum(ROWS)
    row_ids = np.full(int(frame_off[-1]), -1, dtype=np.int64)
    xys = np.zeros((int(frame_off[-1]), 2))
    unknown = UNKNOWN_ID0
    for f in range(F):
        n = ROWS[f]
        ids = np.full(n, -1, dtype=np.int64)
        slots = rng.permutation(n)
        ids[slots[:len(observed[f])]] = observed[f] + 1      # point ids start at 1
        ids[slots[len(observed[f]):len(observed[f]) + 2]] = [unknown, unknown + 1]
        unknown += 2
        if f == FRAME_TWICE:      # a point observed twice in one frame: a second row, on a row that held -1
            ids[slots[-1]] = ids[slots[0]]
        xy = np.stack([rng.uniform(0, WIDTH, n), rng.uniform(0, HEIGHT, n)], axis=1)
        has = (ids > 0) & (ids < UNKNOWN_ID0)
        u, v, _ = project(cams[f], xyz_all[ids[has] - 1])
        xy[has] = np.stack([u, v], axis=1) + 0.7 * rng.standard_normal((int(has.sum()), 2))
        row_ids[frame_off[f]:frame_off[f + 1]], xys[frame_off[f]:frame_off[f + 1]] = ids, xy
    # the point table: COLMAP's image_ids, one entry per observing row, in frame order
    point_frames = {}
    for f in range(F):
        for pid in row_ids[frame_off[f]:frame_off[f + 1]].tolist():
            if 0 < pid < UNKNOWN_ID0:
                point_frames.setdefault(pid, []).append(f)
    pt_ids = np.array(sorted(point_frames), dtype=np.int64)
    pt_xyz = xyz_all[pt_ids - 1]
    pt_err = rng.uniform(0.05, 5.0, len(pt_ids))
    pt_obs = np.array([len(point_frames[p]) for p in pt_ids.tolist()], dtype=np.int64)
    pt_sid = (pt_ids % 5).astype(np.int32)
    s = {"frame_off": frame_off, "point3D_ids": row_ids, "xys": xys, "cams": cams, "point_frames": point_frames, "pt_ids": pt_ids,
         "pt_xyz": pt_xyz, "pt_err": pt_err, "pt_obs": pt_obs, "pt_sid": pt_sid, "seg_ref": SEG_REF, "seed": seed}
    s["results"] = {tag: compress(s, **cfg) for tag, cfg in CONFIGS.items()}
    _scene_cache[seed] = s
    return s


def store_frames(s: dict) -> list:
    """The scene as the frame dicts a ReferenceStore takes (float32 keypoints; the float64 ones go to compress_map as ``xys``)."""
    rng = np.random.default_rng(s["seed"] + 1)
    frames = []
    for f in range(F):
        a, b = int(s["frame_off"][f]), int(s["frame_off"][f + 1])
        d = rng.standard_normal((b - a, 128)).astype(np.float32)
        ids = s["point3D_ids"][a:b]
        at = np.clip(np.searchsorted(s["pt_ids"], ids), 0, len(s["pt_ids"]) - 1)
        known = s["pt_ids"][at] == ids
        frames.append({"id": FRAME_ID0 + f, "keypoints": np.concatenate([s["xys"][a:b], np.ones((b - a, 1))], axis=1).astype(np.float32),
                       "descriptors": d / np.linalg.norm(d, axis=1, keepdims=True), "xyzs": np.where(known[:, None], s["pt_xyz"][at], 0.0),
                       "point3D_ids": ids, "keypoint_segs": np.where(known, s["pt_sid"][at], 0).astype(np.int32), "width": WIDTH,
                       "height": HEIGHT, "qvec": s["cams"][f, 0:4], "tvec": s["cams"][f, 4:7], "intrinsics": s["cams"][f, 7:11]})
    return frames


def store_arguments(s: dict, covisible_frames: int) -> dict:
    """Keyword arguments of ReferenceStore for the scene (beside the frames): frame ids, not indices."""
    return {"seg_ref_frame_ids": {k: [FRAME_ID0 + f for f in v] for k, v in s["seg_ref"].items()},
            "point3D_frame_ids": {p: [FRAME_ID0 + f for f in v] for p, v in s["point_frames"].items()},
            "covisibility_frame": covisible_frames, "point3D_xyzs": {int(p): s["pt_xyz"][i] for i, p in enumerate(s["pt_ids"].tolist())}}


def check_scene(s: dict) -> None:
    """What the scene is for, asserted from the traces: tests/tools/gen_compress_pinned.py re-draws the seed until this passes."""
    rows = np.diff(s["frame_off"])
    assert {ROW_TILE - 1, ROW_TILE, ROW_TILE + 1} <= set(rows.tolist()) and rows.max() > 2 * KPT_TILE and rows.min() < 64 and (rows % 64 != 0).any()
    assert (s["point3D_ids"] == -1).any() and (s["point3D_ids"] >= UNKNOWN_ID0).any()
    a, b = s["frame_off"][FRAME_TWICE], s["frame_off"][FRAME_TWICE + 1]
    ids = s["point3D_ids"][a:b]
    assert len(np.unique(ids[ids > 0])) < int((ids > 0).sum())      # a point observed twice in one frame
    t5, t30, t100 = (s["results"][k]["trace"] for k in ("c5", "c30", "c30n100"))
    assert any(t5["cut"].values()) and not any(t30["cut"].values())
    assert any(c == FRAME_LOSER for _, c in t30["lost_all"])      # a candidate that loses every row
    assert 8 in t30["overwritten"] and 8 in t5["overwritten"]      # a reference frame first retained, in part, as a candidate
    assert t30["appended"] > 0 and t30["outside"] > 0 and len(s["results"]["c30"]["frames"]) < F
    assert len(t100["sparsified"]) >= 3
    for t in (t5, t30, t100):
        for f, counts in t["covis_counts"].items():
            assert len(set(counts)) == len(counts), ("equal covisibility counts in the list of frame", f)
        assert t["radius_margin"] > 1e-6 and t["border_margin"] > 1e-6 and t["depth_margin"] > 1e-6, t
    assert t100["cell_margin"] > 1e-6
