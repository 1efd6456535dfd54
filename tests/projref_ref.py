"""Numpy restatement of the reference's refinement by projection, for the tests of pram_amd.localization.refine.

Written from SingleMap3D.refine_pose_by_projection (localization/singlemap3d.py:367-498) with qvec2rotmat
(colmap_utils/read_write_model.py:556-566), Frame.get_intrinsics (localization/frame.py:154-175) and find_reference_frames
(singlemap3d.py:500-511; tests/refine_ref.py restates it).  Geometry in float64, descriptor distances in fp32, and the matching is
the reference's DENSE formula: every distance, + 100 on the out-of-range ones, the two smallest per keypoint, the ratio test.  The
device gates by range first (include/pram_hip.h, pram_projref_match); that the two agree is what the tests check.

A ``map`` and a ``query`` are tests/refine_ref.py's.  Points are named by their ids, frames by theirs.  Deviations this file shares
with the device: a row with point id -1 or an id the point table does not hold adds nothing to the union (the reference raises
KeyError); fewer than two projected points give no match (the reference's topk(k = 2) raises).

Also the seeded setting the CPU and GPU tests share (projection_scene)."""
from __future__ import annotations

import numpy as np

from tests import pose_ref as PR
from tests import refine_ref as RR


# ---------------------------------------------------------------- the per-point table (point3Ds[pid].xyz / .descriptor / .seg_id)
def point_table(map_: dict, xyzs=None, descriptors=None, sids=None) -> dict:
    """-> dict(ids int64 [n] ascending, xyz float64 [n, 3], desc float32 [n, 128], sid int32 [n]): for every point of
    refine_ref.point_frames the value its dict names, else that of the first row, in map order, carrying the id; neither:
    ValueError."""
    ids = sorted(RR.point_frames(map_))
    first = {}
    for f in map_["frames"]:
        for r, pid in enumerate(np.asarray(f["point3D_ids"]).tolist()):
            if pid != -1 and pid not in first:
                first[pid] = (np.asarray(f["xyzs"], dtype=np.float64)[r], np.asarray(f["descriptors"], dtype=np.float32)[r], int(np.asarray(f["keypoint_segs"])[r]))
    out = {"ids": np.array(ids, dtype=np.int64), "xyz": np.zeros((len(ids), 3)), "desc": np.zeros((len(ids), 128), np.float32), "sid": np.zeros(len(ids), np.int32)}
    for i, pid in enumerate(ids):
        for k, (key, given) in enumerate((("xyz", xyzs), ("desc", descriptors), ("sid", sids))):
            if given is not None and pid in given:
                out[key][i] = given[pid]
            elif pid in first:
                out[key][i] = first[pid][k]
            else:
                raise ValueError(f"point {pid}: no {key}")
    return out


# ---------------------------------------------------------------- geometry
def qvec2rotmat(q):
    q0, q1, q2, q3 = (float(v) for v in q)
    return np.array([[1 - 2 * q2 ** 2 - 2 * q3 ** 2, 2 * q1 * q2 - 2 * q0 * q3, 2 * q3 * q1 + 2 * q0 * q2],
                     [2 * q1 * q2 + 2 * q0 * q3, 1 - 2 * q1 ** 2 - 2 * q3 ** 2, 2 * q2 * q3 - 2 * q0 * q1],
                     [2 * q3 * q1 - 2 * q0 * q2, 2 * q2 * q3 + 2 * q0 * q1, 1 - 2 * q1 ** 2 - 2 * q2 ** 2]])


def intrinsics(cam) -> np.ndarray:
    """Frame.get_intrinsics for a (model_name, width, height, params) tuple; the distortion is left out, as at singlemap3d.py:401."""
    name, prm = cam[0], [float(v) for v in cam[3]]
    if name in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL"):
        fx, fy, cx, cy = prm[0], prm[0], prm[1], prm[2]
    elif name in ("PINHOLE", "OPENCV"):
        fx, fy, cx, cy = prm[:4]
    else:
        raise ValueError(name)
    K = np.identity(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return K


def project(xyz, K, R, t, width, height):
    """singlemap3d.py:405-413 in pram_project_points_f64's operation order -> (u, v, depth, mask)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        c = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
        p = [(K[r, 0] * c[0] + K[r, 1] * c[1]) + K[r, 2] * c[2] for r in range(3)]
        u, v = p[0] / p[2], p[1] / p[2]
        mask = (p[2] > 0) & (p[2] < 100) & (u >= 0) & (u < width) & (v >= 0) & (v < height)
    return u, v, p[2], mask


def union_points(map_: dict, graph: dict, ref_id, table: dict) -> np.ndarray:
    """singlemap3d.py:378-387 -> indices into the point table, ascending (np.unique's order of the ids)."""
    position = {fid: i for i, fid in enumerate(RR.frame_ids(map_))}
    frames = list(graph.get(ref_id, ()))      # a copy: the reference appends to its graph's own list
    if ref_id not in frames:
        frames.append(ref_id)
    ids = []
    for fid in frames:
        ids.extend(np.asarray(map_["frames"][position[fid]]["point3D_ids"]).tolist())
    ids = np.unique(np.array(ids, dtype=np.int64))
    at = np.searchsorted(table["ids"], ids)
    ok = at < len(table["ids"])
    ok[ok] = table["ids"][at[ok]] == ids[ok]
    return at[ok]


# ---------------------------------------------------------------- the dense matching, singlemap3d.py:423-437
def pixel_errors(kpts, uv):
    kpts = np.asarray(kpts, dtype=np.float32)[:, :2]
    err = kpts[..., None] - np.asarray(uv, dtype=np.float64)[None]      # float32 - float64 -> float64 [M, 2, N]
    return np.sqrt(np.sum(err ** 2, axis=1))


def dense_match(kpts, descs, uv, pt_descs, threshold: float) -> dict:
    """kpts float32 [M, 2], descs float32 [M, 128], uv float64 [2, N], pt_descs float32 [N, 128] -> ratio_mask bool [M], ids [M]
    (nearest candidate), dists float32 [M, 2] (with the + 100 where it applies), n_in [M] (in-range candidates) and err [M, N]."""
    m, n = np.asarray(descs).shape[0], np.asarray(pt_descs).shape[0]
    err = pixel_errors(kpts, uv) if n else np.zeros((m, 0))
    if n < 2:      # topk(k = 2) has nothing to take: no match; the single candidate's distance is still reported
        d = np.full((m, 2), np.inf, np.float32)
        if n == 1:
            q1, d1 = np.asarray(descs, dtype=np.float32), np.asarray(pt_descs, dtype=np.float32)
            d[:, 0] = np.sqrt(np.float32(2) - np.float32(2) * (q1 @ d1.T)[:, 0] + np.float32(1e-6)) + np.where(err[:, 0] >= 2 * threshold, np.float32(100), np.float32(0))
        return {"ratio_mask": np.zeros(m, bool), "ids": np.zeros(m, np.int64) if n else np.full(m, -1, np.int64), "dists": d, "n_in": (err < 2 * threshold).sum(1),
                "err": err}
    out_of_range = err >= 2 * threshold
    q, d = np.asarray(descs, dtype=np.float32), np.asarray(pt_descs, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(np.float32(2) - np.float32(2) * (q @ d.T) + np.float32(1e-6)).astype(np.float32)
    dist[out_of_range] = dist[out_of_range] + np.float32(100)
    order = np.argsort(dist, axis=1, kind="stable")[:, :2]      # topk(k = 2, largest = False); equal distances: lowest index first
    dists = np.take_along_axis(dist, order, 1)
    with np.errstate(all="ignore"):
        ratio_mask = (dists[:, 0] / dists[:, 1] <= np.float32(0.995)) & (dists[:, 0] < 100)
    return {"ratio_mask": ratio_mask, "ids": order[:, 0], "dists": dists, "n_in": (~out_of_range).sum(1), "err": err, "dist": dist}


def gated_view(dm: dict):
    """What pram_projref_match reports, read off dense_match's result: best (-1: none in range), d0 / d1 (+inf: none), accept."""
    d = dm["dists"].astype(np.float32).copy()
    n_in = dm["n_in"]
    d[n_in < 1, 0] = np.inf
    d[n_in < 2, 1] = np.inf
    return np.where(n_in >= 1, dm["ids"], -1).astype(np.int32), d[:, 0], d[:, 1], dm["ratio_mask"].astype(np.uint8)


def refine_by_projection(query: dict, map_: dict, located: dict, cam, solver, *, threshold: float, covisibility_frame: int, graph: dict = None,
                         table: dict = None) -> dict:
    """refine_pose_by_projection for one located query.  located: reference_frame_id, qvec (w, x, y, z), tvec.  solver(keypoints,
    xyzs) -> dict(success, inliers, ...).  -> the reference's lists (matched_keypoints, matched_keypoint_ids, matched_xyzs,
    matched_point3D_ids, matched_sids), the solver's result, refinement_reference_frame_ids, reference_frame_id, and what the
    tests look at on the way: union (point-table indices), u, v, depth, mask over the union, cand (indices of the kept), dm."""
    graph = RR.covisibility_graph(map_, covisibility_frame) if graph is None else graph
    table = point_table(map_) if table is None else table
    union = union_points(map_, graph, located["reference_frame_id"], table)
    R, t = qvec2rotmat(located["qvec"]), np.asarray(located["tvec"], dtype=np.float64)
    u, v, depth, mask = project(table["xyz"][union], intrinsics(cam), R, t, cam[1], cam[2])
    cand = union[mask]
    n = query["count"] if "count" in query else len(query["keypoints"])
    kp, de = np.asarray(query["keypoints"], dtype=np.float32)[:n], np.asarray(query["descriptors"], dtype=np.float32)[:n]
    dm = dense_match(kp, de, np.stack([u[mask], v[mask]]), table["desc"][cand], threshold)
    rm = dm["ratio_mask"]
    pts = cand[dm["ids"][rm]] if rm.any() else np.zeros(0, dtype=np.int64)
    out = {"matched_keypoints": kp[rm][:, :2], "matched_keypoint_ids": np.where(rm)[0].astype(np.int64), "matched_xyzs": table["xyz"][pts],
           "matched_point3D_ids": table["ids"][pts], "matched_sids": table["sid"][pts], "union": union, "u": u, "v": v, "depth": depth, "mask": mask,
           "cand": cand, "dm": dm}
    ret = solver(out["matched_keypoints"], out["matched_xyzs"])
    out.update(ret)
    ids = out["matched_point3D_ids"]
    best = RR.find_reference_frames(map_, ids[np.asarray(ret["inliers"], dtype=bool)] if ret["success"] else ids, graph.keys())
    out["refinement_reference_frame_ids"] = best[:covisibility_frame]
    out["reference_frame_id"] = best[0] if best else located["reference_frame_id"]
    return out


def margins(res: dict, cam, threshold: float) -> dict:
    """How far the decisions of one refine_by_projection result stand from their bounds: the smallest distance of a pixel error
    from 2 * threshold, of u, v, depth (over the whole union) from a frustum bound, of d0 / d1 from 0.995 and the smallest
    d1 - d0 (the two smallest in-range distances), the last two over keypoints with two or more in-range candidates."""
    dm = res["dm"]
    inf = float("inf")
    m = {"range": float(np.abs(dm["err"] - 2 * threshold).min()) if dm["err"].size else inf, "frustum": inf, "ratio": inf, "gap": inf}
    with np.errstate(all="ignore"):
        for val, bounds in ((res["u"], (0.0, cam[1])), (res["v"], (0.0, cam[2])), (res["depth"], (0.0, 100.0))):
            for bnd in bounds:
                if val.size:
                    m["frustum"] = min(m["frustum"], float(np.abs(val - bnd).min()))
    two = dm["n_in"] >= 2
    if two.any():
        d = dm["dists"][two].astype(np.float64)
        m["ratio"] = float(np.abs(d[:, 0] / d[:, 1] - 0.995).min())
        m["gap"] = float((d[:, 1] - d[:, 0]).min())
    return m


# ---------------------------------------------------------------- the shared setting
# localization.threshold.  The reference's configs say 12; at 12 px the restatement itself (pose_ref.estimate_pose on its own lists)
# leaves entry 0 1.02 degrees from the planted camera, because clutter keypoints matched to a stranger within 24 px pass the
# RANSAC bound; at 8 px every entry ends within 0.4 degrees, and keypoints with two and more in-range candidates remain
THRESHOLD = 8.0
SCENE_SEED = 7
# batch entry -> (query of covisible_scene, frame id the localisation kept, enabled); entry 5 is the empty query (not located),
# entry 6 a located query that is switched off.  Query 2 has 64 keypoints, 52 of them planted, so the entries that can reach 64
# matches are those of queries 0 and 1: 0, 1, 4 (and 6)
CASES = ((0, 101, 1), (1, 105, 1), (2, 107, 1), (3, 107, 1), (0, 100, 1), (4, None, 1), (1, 104, 0))
UNLISTED = (101,)           # frames taken out of every point's frame list: they are not in their own covisible list
POSE_NOISE = (0.002, 0.02)  # radians, metres: how far the localisation's pose stands from the planted camera


def projection_scene(seed: int = SCENE_SEED):
    """covisible_scene with explicit point3D_frame_ids — the rows' own lists without the UNLISTED frames, so that frame 101's
    covisible list does not hold 101 and the reference appends it (singlemap3d.py:380-381) — plus, per entry of CASES, the
    localisation a refinement starts from: the planted camera of the query turned by about 0.1 degrees and moved by centimetres.
    -> (map, queries, planted, located): located[i] = dict(query, reference_frame_id, qvec, tvec, enable) or None for the entry
    that is not located."""
    map_, queries, planted = RR.covisible_scene(seed)
    map_ = dict(map_, point3D_frame_ids={pid: [f for f in fr if f not in UNLISTED] for pid, fr in RR.point_frames(map_).items()})
    graph = RR.covisibility_graph(map_, RR.COVIS)
    assert 101 not in graph[101] and 100 in graph[100] and 105 in graph[105]
    rng = np.random.default_rng(seed + 1000)
    located = []
    for b, ref_id, on in CASES:
        w = rng.standard_normal(3) * POSE_NOISE[0]
        dt = rng.standard_normal(3) * POSE_NOISE[1]
        if ref_id is None:
            located.append(None)
            continue
        dR = PR.rodrigues(w)
        located.append({"query": b, "reference_frame_id": ref_id, "qvec": PR.rot_to_qvec(dR @ planted[b]["R"]), "tvec": dR @ planted[b]["t"] + dt,
                        "enable": bool(on)})
    return map_, queries, planted, located


# ---------------------------------------------------------------- crafted inputs for the kernels on their own
MARK_CAMERAS = (("SIMPLE_PINHOLE", 640, 480, [500.0, 320.0, 240.0]), ("PINHOLE", 600, 500, [480.0, 510.0, 300.0, 250.0]),
                ("SIMPLE_RADIAL", 640, 480, [520.0, 318.0, 242.0, -0.06]), ("RADIAL", 320, 240, [260.0, 160.0, 120.0, -0.05, 0.01]),
                ("OPENCV", 640, 480, [540.0, 548.0, 316.0, 244.0, -0.08, 0.03, 0.0008, -0.0006]))
# query -> (frame id the localisation kept, or None; kept candidate 0 / 1; enabled)
MARK_QUERIES = ((50, 0, 1), (51, 1, 1), (None, 0, 1), (52, 1, 0), (53, 0, 1), (54, 1, 1), (50, 1, 1))


def mark_map(n_points: int, seed: int):
    """Six frames of 0 .. 2 n_points / 3 + 5 rows over n_points map points, every point in one to three frames; a few rows with id -1
    and a few with ids the point table does not hold; frame 55 is nobody's reference frame; frame 50 is taken out of every point's
    list, so it is not in its own covisible list.  Points lie in a box around the optical axis of a camera at the origin: in
    front and behind, nearer and farther than 100 m, inside and outside every image edge.
    -> (map, queries): queries[i] = dict(reference_frame_id or None, kept, enable, cam, qvec, tvec); query 5 looks away from the
    box (nothing projects)."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.permutation(50 * n_points + 100)[:n_points] + 7).astype(np.int64)
    unknown = np.array([ids.max() + 11, ids.max() + 12, 3], dtype=np.int64)
    xyz = np.stack([rng.uniform(-40, 40, n_points), rng.uniform(-30, 30, n_points), rng.uniform(-30, 160, n_points)], 1)
    desc = rng.standard_normal((n_points, 128)).astype(np.float32)
    sid = rng.integers(0, 9, n_points).astype(np.int32)
    member = [[] for _ in range(6)]
    for i in range(n_points):
        for f in rng.permutation(6)[:rng.integers(1, 4)]:
            member[f].append(i)
    frames, lists = [], {int(p): [] for p in ids}
    for f in range(6):
        own = np.array(member[f], dtype=np.int64)
        pid = np.concatenate([ids[own], np.full(2, -1), unknown[:1 + f % 3]]).astype(np.int64)
        at = np.concatenate([own, np.zeros(len(pid) - len(own), dtype=np.int64)])
        perm = rng.permutation(len(pid))
        frames.append({"id": 50 + f, "keypoints": np.zeros((len(pid), 3), np.float32), "descriptors": desc[at][perm], "xyzs": xyz[at][perm],
                       "point3D_ids": pid[perm], "keypoint_segs": sid[at][perm], "width": 640, "height": 480})
        for i in own:
            if f != 0:
                lists[int(ids[i])].append(50 + f)
    map_ = {"frames": frames, "seg_ref_frame_ids": {l: [50 + l, 50 + (l + 1) % 5] for l in range(5)}, "start_sid": 0, "point3D_frame_ids": lists}
    queries = []
    for i, (ref_id, kept, on) in enumerate(MARK_QUERIES):
        w = rng.standard_normal(3) * 0.05
        if i == 5:
            w = np.array([0.0, np.pi, 0.0])      # turned round: the whole box is behind or beyond
        queries.append({"reference_frame_id": ref_id, "kept": kept, "enable": bool(on), "cam": MARK_CAMERAS[i % len(MARK_CAMERAS)],
                        "qvec": PR.rot_to_qvec(PR.rodrigues(w)), "tvec": rng.standard_normal(3) * (0.5 if i != 5 else 0.0) - (np.array([0, 0, 200.0]) if i == 5 else 0)})
    return map_, queries


def mark_expected(map_: dict, queries, n_cov: int, table: dict = None):
    """Per query (None: not located or not enabled) the union, the kept points and their (u, v), plus the margins of the frustum
    decisions."""
    graph = RR.covisibility_graph(map_, n_cov)
    table = point_table(map_) if table is None else table
    out = []
    for q in queries:
        if q["reference_frame_id"] is None or not q["enable"]:
            out.append(None)
            continue
        union = union_points(map_, graph, q["reference_frame_id"], table)
        cam = q["cam"]
        u, v, depth, mask = project(table["xyz"][union], intrinsics(cam), qvec2rotmat(q["qvec"]), np.asarray(q["tvec"], dtype=np.float64), cam[1], cam[2])
        out.append({"union": union, "cand": union[mask], "uv": np.stack([u[mask], v[mask]]), "u": u, "v": v, "depth": depth, "mask": mask,
                    "listed": q["reference_frame_id"] in graph[q["reference_frame_id"]], "list_len": len(graph[q["reference_frame_id"]])})
    return out


MATCH_COUNTS = (0, 1, 63, 64, 65, 192, 150)           # keypoints per query; 192 is the padded width
MATCH_CANDS = (65, 3000, 64, 2, 63, 1, 0)            # candidates per query; rolled by the tests so that every pair of sizes meets
MATCH_N, MATCH_POINTS, MATCH_THRESHOLD = 192, 4000, 12.0


def match_case(seed: int, roll: int = 0) -> dict:
    """Crafted inputs for pram_projref_match: 7 queries padded to 192 keypoints, candidate lists of 0 .. 3000 points drawn from a
    table of 4000 unit descriptors, projections uniform in a 640 x 480 image (few candidates: a keypoint has 0, 1 or 2 in range;
    3000: many), keypoints on integer pixels, a third of them noisy twins of a candidate placed within range of it."""
    rng = np.random.default_rng(seed)
    B, N = len(MATCH_COUNTS), MATCH_N
    cands = list(np.roll(MATCH_CANDS, roll))
    cap = max(cands)
    unit = lambda x: (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)
    pt_desc = unit(rng.standard_normal((MATCH_POINTS, 128)))
    cand_pt = np.full((B, cap), -1, dtype=np.int32)
    cand_uv = np.full((B, 2, cap), np.nan)
    kpts = np.floor(rng.uniform(0, [640, 480], (B, N, 2))).astype(np.float32)
    desc = unit(rng.standard_normal((B, N, 128)))
    for b in range(B):
        n = cands[b]
        cand_pt[b, :n] = np.sort(rng.permutation(MATCH_POINTS)[:n])
        cand_uv[b, :, :n] = rng.uniform(0, [[640], [480]], (2, n))
        if n:
            for i in range(0, N, 3):
                c = rng.integers(0, n)
                kpts[b, i] = np.floor(cand_uv[b, :, c] + rng.uniform(-6, 6, 2))
                desc[b, i] = unit(pt_desc[cand_pt[b, c]] + 0.3 / np.sqrt(128.0) * rng.standard_normal(128))
    return {"kpts": kpts, "desc": desc, "counts": np.array(MATCH_COUNTS, dtype=np.int32), "cand_pt": cand_pt, "cand_uv": cand_uv,
            "n_cand": np.array(cands, dtype=np.int32), "pt_desc": pt_desc, "threshold": MATCH_THRESHOLD}


def match_expected(case: dict):
    """Per query dense_match over its own keypoints and candidates -> list of its dicts."""
    out = []
    for b in range(len(case["counts"])):
        m, n = int(case["counts"][b]), int(case["n_cand"][b])
        out.append(dense_match(case["kpts"][b, :m], case["desc"][b, :m], case["cand_uv"][b, :, :n], case["pt_desc"][case["cand_pt"][b, :n]], case["threshold"]))
    return out


def match_margins(dm: dict, threshold: float) -> dict:
    return margins({"dm": dm, "u": np.zeros(0), "v": np.zeros(0), "depth": np.zeros(0)}, (None, 1, 1), threshold)
