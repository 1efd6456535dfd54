"""Numpy restatement of the reference's tracker, for the tests of pram_amd.localization.tracker.

Written from Tracker.track_last_frame, run and verify_and_update (localization/tracker.py:37-233), Frame.
initialize_localization_variables and update_point3ds (localization/frame.py:84-89, 191-195) and the tracker / relocalisation
switch of the loops (localization/loc_by_rec_online.py:181-197).  Plain host loops over plain numpy.  A ``frame`` is a dict with
keypoints [n, 2], scores [n], descriptors [n, 128], width, height and, once located, seg_ids / point3D_ids / xyzs [n] and
reference_frame_id.  The matcher, the solver, the refinement and the relocalisation are callables, so the same code runs on
numpy stand-ins (the CPU tests) and on what the device produced (the GPU tests).

Also the seeded sequence the CPU and GPU tests share (sequence_scene)."""
from __future__ import annotations

import numpy as np

from tests import cand_ref as CR
from tests import pose_ref as PR
from tests import refine_ref as RR

LIST_KEYS = RR.STACK_KEYS


def initialize_localization_variables(frame: dict, seg_ids=None) -> dict:
    """frame.py:191-195; seg_ids: the frame's own labels (add_segmentations, frame.py:121), None: -1."""
    n = int(np.asarray(frame["keypoints"]).shape[0])
    frame["seg_ids"] = np.full(n, -1, dtype=np.int32) if seg_ids is None else np.asarray(seg_ids, dtype=np.int32)[:n].copy()
    frame["point3D_ids"] = np.full(n, -1, dtype=np.int64)
    frame["xyzs"] = np.zeros((n, 3), dtype=np.float64)
    return frame


def update_point3ds(frame: dict, lists: dict) -> dict:
    """frame.py:84-89: numpy's fancy assignment, so of the rows naming one keypoint the last wins."""
    ids = np.asarray(lists["matched_keypoint_ids"], dtype=np.int64)
    frame["xyzs"][ids] = np.asarray(lists["matched_xyzs"], dtype=np.float64)
    frame["seg_ids"][ids] = np.asarray(lists["matched_sids"], dtype=np.int32)
    frame["point3D_ids"][ids] = np.asarray(lists["matched_point3D_ids"], dtype=np.int64)
    return frame


def track_last_frame(curr: dict, last: dict, matcher) -> dict:
    """tracker.py:162-210, up to the solver: matcher(data) -> matches0 int64 [n]; -> the six lists plus matches0."""
    ck = np.asarray(curr["keypoints"], dtype=np.float32)
    lk = np.asarray(last["keypoints"], dtype=np.float32)
    data = {"descriptors0": curr["descriptors"], "keypoints0": ck, "scores0": curr["scores"], "image_shape0": (1, 3, curr["width"], curr["height"]),
            "descriptors1": last["descriptors"], "keypoints1": lk, "scores1": last["scores"], "image_shape1": (1, 3, last["width"], last["height"])}
    ind = np.asarray(matcher(data), dtype=np.int64)
    valid = ind >= 0
    rows = ind[valid]
    p3d = np.asarray(last["point3D_ids"])[rows]
    has = p3d >= 0
    return {"matches0": ind, "matched_keypoints": ck[valid][has], "matched_keypoint_ids": np.arange(ck.shape[0])[valid][has],
            "matched_xyzs": np.asarray(last["xyzs"], dtype=np.float64)[rows][has], "matched_point3D_ids": p3d[has],
            "matched_sids": np.asarray(last["seg_ids"])[rows][has], "matched_ref_keypoints": lk[rows][has]}


def take(lists: dict, mask) -> dict:
    """ret[...][inliers] (tracker.py:154-160, multimap3d.py:263-267)."""
    mask = np.asarray(mask, dtype=bool)
    return {k: np.asarray(lists[k])[mask] for k in LIST_KEYS if lists.get(k) is not None}


class TrackerLoop:
    """Tracker.run inside the loop of loc_by_rec_online.py:181-197 for n_streams independent streams.

    step(queries, streams, matcher, solver, refiner, relocalizer, seg_ids): queries[b] a frame dict, streams[b] its stream;
    matcher(b, data) -> matches0; solver(b, lists) -> dict(success, num_inliers, inliers, qvec, tvec); refiner(b, frame, located,
    ret) -> None or the refinement's dict (success, num_inliers, inliers, the lists, reference_frame_id), located = the tracker's
    inlier rows with reference_frame_id and tracking_status True; relocalizer(i, b, frame) for the i-th query handed to it -> dict(
    success, reference_frame_id, the lists of the kept candidate, refinement = None or a dict as above).  -> per query dict(source,
    success, reference_frame_id, lists (what is committed), tracking).  lost = not success (tracker.py:120 is repaired by the loop)."""

    def __init__(self, n_streams: int, *, min_inliers: int, refine_below: int = 256):
        self.lost = [True] * n_streams
        self.last = [None] * n_streams
        self.min_inliers, self.refine_below = int(min_inliers), int(refine_below)

    def step(self, queries, streams, matcher, solver, refiner, relocalizer, seg_ids=None):
        out, rest = [None] * len(queries), []
        for b, (q, s) in enumerate(zip(queries, streams)):
            if self.lost[s]:
                rest.append(b)
                continue
            lists = track_last_frame(q, self.last[s], lambda d: matcher(b, d))
            ret = solver(b, lists)
            tracking = {"lists": lists, "ret": ret}
            ok = bool(ret["success"]) and int(ret["num_inliers"]) >= self.min_inliers      # verify_and_update
            source, commit, fid = "track", None, self.last[s]["reference_frame_id"]
            if ok:
                commit = take(lists, ret["inliers"])
                if int(ret["num_inliers"]) < self.refine_below:      # tracker.py:85-94
                    x = refiner(b, q, dict(commit, reference_frame_id=fid, tracking_status=True), ret)
                    tracking["refinement"] = x
                    if x is not None and x["success"]:      # a refinement with success False changes nothing
                        if int(x["num_inliers"]) < self.min_inliers:
                            ok = False
                        else:
                            source, commit, fid = "track+refine", take(x, x["inliers"]), x["reference_frame_id"]
            if not ok:
                self.lost[s] = True
                rest.append(b)
                out[b] = {"source": None, "success": False, "tracking": tracking}
                continue
            out[b] = {"source": source, "success": True, "reference_frame_id": fid, "lists": commit, "tracking": tracking}
        rest.sort()
        for i, b in enumerate(rest):
            q, s = queries[b], streams[b]
            r = relocalizer(i, b, q)
            tracking = None if out[b] is None else out[b]["tracking"]
            if not r["success"]:
                self.lost[s] = True
                out[b] = {"source": None, "success": False, "tracking": tracking}
                continue
            x = r.get("refinement")
            if x is not None and x["success"]:      # multimap3d.py:259-271
                commit, fid = take(x, x["inliers"]), x["reference_frame_id"]
            else:                                    # update_query_frame keeps the outliers (multimap3d.py:315-328)
                commit, fid = {k: np.asarray(r[k]) for k in LIST_KEYS if r.get(k) is not None}, r["reference_frame_id"]
            out[b] = {"source": "relocalize", "success": True, "reference_frame_id": fid, "lists": commit, "tracking": tracking}
        for b, (q, s) in enumerate(zip(queries, streams)):      # loc_by_rec_online.py:193-197
            if not out[b]["success"]:
                continue
            frame = dict(q)
            initialize_localization_variables(frame, None if seg_ids is None else seg_ids[b])
            update_point3ds(frame, out[b]["lists"])
            frame["reference_frame_id"] = out[b]["reference_frame_id"]
            self.last[s], self.lost[s] = frame, False
        return out


def state_arrays(loop: TrackerLoop, n_max: int, frame_index: dict) -> dict:
    """What a TrackState holds after the same steps: per slot count, ref_frame (store index), frame_norm, and the frame's arrays
    padded to n_max (xyz 0, point id -1, seg id -1 beyond the count; keypoints / scores / descriptors are compared on the first
    count rows only).  A slot that was never committed: count 0, ref_frame -1, frame_norm (0, 0, 1), no points."""
    S = len(loop.last)
    st = {"counts": np.zeros(S, np.int32), "ref_frame": np.full(S, -1, np.int32), "frame_norm": np.tile(np.array([0, 0, 1], np.float32), (S, 1)),
          "keypoints": np.zeros((S, n_max, 2), np.float32), "scores": np.zeros((S, n_max), np.float32), "descriptors": np.zeros((S, n_max, 128), np.float32),
          "xyzs": np.zeros((S, n_max, 3), np.float64), "point3D_ids": np.full((S, n_max), -1, np.int64), "seg_ids": np.full((S, n_max), -1, np.int32)}
    for s, f in enumerate(loop.last):
        if f is None:
            continue
        n = int(np.asarray(f["keypoints"]).shape[0])
        st["counts"][s], st["ref_frame"][s] = n, frame_index[f["reference_frame_id"]]
        st["frame_norm"][s] = np.array(CR.norm_constants(f["width"], f["height"]), dtype=np.float32)
        st["keypoints"][s, :n], st["scores"][s, :n], st["descriptors"][s, :n] = f["keypoints"], f["scores"], f["descriptors"]
        st["xyzs"][s, :n], st["point3D_ids"][s, :n], st["seg_ids"][s, :n] = f["xyzs"], f["point3D_ids"], f["seg_ids"]
    return st


# ---------------------------------------------------------------- the seeded sequence
N_STREAMS, N_FRAMES = 4, 3
# per stream: (first point, points, clutter) of frame 0, counted inside the run of points refine_ref.covisible_scene planted a
# camera for (its QUERY_WINDOWS 0, 1, 2), and the covisible_scene query whose planted camera the stream starts from
STREAM_WINDOWS = ((4, 106, 16, 0), (6, 56, 10, 1), (0, 44, 8, 2), (0, 0, 0, 3))
WINDOW_STEP = 3                     # the window moves by three pool points per frame
JUMP = (2, 2, (8, 100, 12, 0))      # stream 2, frame 2: a distant window (stream 0's region), so tracking fails there
SCENE_SEED = 7


def _camera_step(rng):
    """A small motion per frame: about 0.2 degrees and 5 cm."""
    return PR.rodrigues(rng.standard_normal(3) * 0.0035), rng.standard_normal(3) * 0.05


def sequence_scene(seed: int = SCENE_SEED, noise: float = 0.25, noise_px: float = 0.3):
    """Four streams of three frames over refine_ref.covisible_scene's map.  A frame sees a window of the pool through its stream's
    camera, which starts at the camera covisible_scene planted for that window and moves a little per frame: its keypoints are
    the projections (minus 0.5, plus Gaussian noise) of the window's points, which the map's frames hold with the same xyz, plus
    clutter; descriptors are the pool's plus noise; the logits peak at the point's landmark.  Stream 0: a wide window (112 points),
    it tracks throughout.  Stream 1: a narrow one (56), so its tracking inliers stay below a ``refine_below`` placed between the
    two.  Stream 2: frame 2 jumps to a distant window, so tracking fails and it relocalises.  Stream 3: no keypoints, never located.
    -> (map, frames, planted): frames[t][s] a cand_ref query (padded to refine_ref.N_PAD), planted[t][s] = dict(cam, R, t)."""
    map_, _, planted0 = RR.covisible_scene()
    rng = np.random.default_rng(seed)
    w, h = RR.CAMERA
    # the pool, recovered from the map's frames: point id -> (xyz, landmark, a descriptor)
    pool = {}
    for f in map_["frames"]:
        for r, pid in enumerate(np.asarray(f["point3D_ids"]).tolist()):
            if pid != -1 and pid not in pool:
                pool[pid] = (np.asarray(f["xyzs"])[r], int(np.asarray(f["keypoint_segs"])[r]), np.asarray(f["descriptors"])[r])
    # the points covisible_scene planted for its query b are those its planted camera sees at the planted depth of 3 .. 30 m (the
    # rest of the pool lies hundreds of metres from every camera); a stream's window is a run of them in ascending point id
    windows = []
    for b in range(3):
        cam = PR.PLANTED_CAMERAS[b % len(PR.PLANTED_CAMERAS)]
        model, params = PR.camera_row(cam)
        ids = np.array(sorted(pool), dtype=np.int64)
        px, z = PR.project(np.array([pool[int(p)][0] for p in ids]), planted0[b]["R"], planted0[b]["t"], model, params)
        seen = (z > 2.5) & (z < 30.5) & (px[:, 0] >= 0) & (px[:, 0] < w) & (px[:, 1] >= 0) & (px[:, 1] < h)
        windows.append(ids[seen].tolist())
        assert len(windows[b]) == RR.QUERY_WINDOWS[b][1], (b, len(windows[b]))
    frames, planted = [], []
    cams = {}
    for t in range(N_FRAMES):
        row, prow = [], []
        for s, (first, n_pts, n_clutter, src) in enumerate(STREAM_WINDOWS):
            if s not in cams:
                cams[s] = (planted0[src]["R"].copy(), planted0[src]["t"].copy())
            if (s, t) == JUMP[:2]:
                first, n_pts, n_clutter, src = JUMP[2]
                cams[s] = (planted0[src]["R"].copy(), planted0[src]["t"].copy())
            dR, dt = _camera_step(rng)
            R, tv = dR @ cams[s][0], dR @ cams[s][1] + dt      # the camera frame turns and shifts: x_cam -> dR x_cam + dt
            cams[s] = (R, tv)
            cam = PR.PLANTED_CAMERAS[s % len(PR.PLANTED_CAMERAS)]
            model, params = PR.camera_row(cam)
            own = windows[src][first + WINDOW_STEP * t:first + WINDOW_STEP * t + n_pts] if n_pts else []
            assert len(own) == n_pts
            xyz = np.array([pool[p][0] for p in own]).reshape(-1, 3)
            px, z = PR.project(xyz, R, tv, model, params) if n_pts else (np.zeros((0, 2)), np.zeros(0))
            px = px - 0.5 + noise_px * rng.standard_normal(px.shape)
            keep = (z > 0) & (px[:, 0] >= 0) & (px[:, 0] < w - 1) & (px[:, 1] >= 0) & (px[:, 1] < h - 1)
            own, px = [p for p, k in zip(own, keep) if k], px[keep]
            n_own = len(own)
            n = n_own + n_clutter
            d = np.concatenate([CR._unit(np.array([pool[p][2] for p in own]).reshape(-1, 128) + noise / np.sqrt(128.0) * rng.standard_normal((n_own, 128))),
                                CR._unit(rng.standard_normal((n_clutter, 128)))]) if n else np.zeros((0, 128))
            k = np.concatenate([px, np.stack([rng.uniform(4, w - 4, n_clutter), rng.uniform(4, h - 4, n_clutter)], 1)])
            cls = np.concatenate([np.array([pool[p][1] for p in own], dtype=np.int64) + 1, np.zeros(n_clutter, dtype=np.int64)])
            pid = np.concatenate([np.array(own, dtype=np.int64), np.full(n_clutter, -1, dtype=np.int64)])
            perm = rng.permutation(n)
            d, k, cls, pid = d[perm].reshape(n, 128), k[perm].reshape(n, 2), cls[perm], pid[perm]
            seg = rng.standard_normal((n, RR.N_CLASS)).astype(np.float32)
            seg[np.arange(n), cls] += 8.0
            pad = lambda a: np.concatenate([a, np.zeros((RR.N_PAD - n,) + a.shape[1:], dtype=a.dtype)])
            q = {"keypoints": k.astype(np.float32), "scores": rng.uniform(0, 1, n).astype(np.float32), "descriptors": d.astype(np.float32),
                 "segmentations": seg, "seg_ids": (np.argmax(seg, 1) - 1).astype(np.int32) if n else np.zeros(0, np.int32), "width": w, "height": h,
                 "pool": pid, "count": n}
            q["padded"] = {kk: pad(q[kk]) for kk in ("keypoints", "scores", "descriptors", "segmentations")}
            row.append(q)
            prow.append({"cam": cam, "R": R, "t": tv})
        frames.append(row)
        planted.append(prow)
    return map_, frames, planted


def real(q: dict) -> dict:
    """A scene query without its padding, as a frame."""
    return {k: v for k, v in q.items() if k != "padded"}


def planted_solver(planted, threshold: float):
    """A stand-in for the pose stage on the CPU: the planted camera is the answer, a row is an inlier when it reprojects within
    ``threshold`` pixels of its keypoint; fewer than 3 rows, or fewer than 3 inliers: failure."""
    def solve(lists, p):
        kp, xyz = np.asarray(lists["matched_keypoints"], dtype=np.float64).reshape(-1, 2), np.asarray(lists["matched_xyzs"]).reshape(-1, 3)
        n = kp.shape[0]
        fail = {"success": False, "num_inliers": 0, "inliers": np.zeros(n, dtype=bool), "qvec": np.zeros(4), "tvec": np.zeros(3)}
        if n < 3:
            return fail
        model, params = PR.camera_row(p["cam"])
        px, z = PR.project(xyz, p["R"], p["t"], model, params)
        inl = (z > 0) & (np.linalg.norm(px - (kp + 0.5), axis=1) <= threshold)
        if inl.sum() < 3:
            return fail
        return {"success": True, "num_inliers": int(inl.sum()), "inliers": inl, "qvec": PR.rot_to_qvec(p["R"]), "tvec": p["t"].copy()}
    return solve


# ---------------------------------------------------------------- the cases pinned by running the reference
def pinned_cases(seed: int = SCENE_SEED):
    """The inputs of tests/tools/gen_track_pinned.py and of the test that replays its fixture, rebuilt from the seed: per case a
    last frame (a scene frame whose pool keypoints carry their map point, every fifth of them none), the current frame, the
    recorded matches0 — the mutual nearest neighbours, then some set to -1 and some moved onto rows without a point — and an
    update list with repeated keypoint ids (the solver's rows, then its first rows again with other values, as the matching
    refinement stacks one keypoint once per covisible frame)."""
    map_, frames, _ = sequence_scene(seed)
    point = {}
    for f in map_["frames"]:
        for r, pid in enumerate(np.asarray(f["point3D_ids"]).tolist()):
            point.setdefault(pid, (np.asarray(f["xyzs"])[r], int(np.asarray(f["keypoint_segs"])[r])))
    rng = np.random.default_rng(seed + 1)
    mm = RR.mnn_matcher()
    cases = []
    for s, t in ((0, 1), (1, 2), (2, 1), (2, 2)):
        last, curr = real(frames[t - 1][s]), real(frames[t][s])
        initialize_localization_variables(last, last["seg_ids"])
        has = np.nonzero(last["pool"] >= 0)[0]
        has = has[np.arange(len(has)) % 5 != 4]
        update_point3ds(last, {"matched_keypoint_ids": has, "matched_xyzs": np.array([point[int(p)][0] for p in last["pool"][has]]).reshape(-1, 3),
                               "matched_sids": np.array([point[int(p)][1] for p in last["pool"][has]], dtype=np.int32),
                               "matched_point3D_ids": last["pool"][has]})
        last["reference_frame_id"] = 100 + s
        m0 = track_last_frame(curr, last, mm)["matches0"].copy()
        hit = np.nonzero(m0 >= 0)[0]
        m0[hit[::7]] = -1
        bare = np.nonzero(last["point3D_ids"] < 0)[0]
        if len(hit) > 3 and len(bare):
            m0[hit[1::9]] = bare[rng.integers(0, len(bare), len(hit[1::9]))]
        lists = track_last_frame(curr, last, lambda d: m0)
        n = len(lists["matched_keypoint_ids"])
        k = min(10, n)
        again = {"matched_keypoint_ids": lists["matched_keypoint_ids"][:k][::-1].copy(), "matched_xyzs": lists["matched_xyzs"][:k] + 1.0,
                 "matched_sids": lists["matched_sids"][:k] + 50, "matched_point3D_ids": lists["matched_point3D_ids"][:k] + 7}
        update = {key: np.concatenate([lists[key], again[key], again[key][:k // 2] if key != "matched_xyzs" else again[key][:k // 2] - 3.0])
                  for key in again}
        cases.append({"stream": s, "frame": t, "last": last, "curr": curr, "matches0": m0, "update": update})
    return cases
