"""Numpy restatement of the reference's candidate loop, for the tests of pram_amd.localization.candidates.

Written from the behaviour of MultiMap3D.process_segmentations / run (localization/multimap3d.py:348-379, 110-145),
SingleMap3D.check_semantic_consistency / localize_with_ref_frame (singlemap3d.py:513-532, 127-162) and RefFrame.get_keypoints /
get_keypoints_by_sid (refframe.py:34-75).  Plain host code over plain numpy: a ``map`` is dict(frames = list of dicts as
ReferenceStore takes them, seg_ref_frame_ids, start_sid); a ``query`` is dict(keypoints [n, 2], scores [n], descriptors [n, 128],
segmentations [n, C], seg_ids [n], width, height).  The matcher is a callable data-dict -> matches0 (numpy int64 [m]).

Also the seeded synthetic map / queries the GPU tests and the timing script share (make_map, make_query)."""
from __future__ import annotations

import numpy as np


def process_segmentations(segs: np.ndarray, topk: int):
    """-> [(class id, token ids, mean score)], best first: rank by rank over each token's classes sorted by score (descending,
    ties by ascending class), the classes seen at that rank that are not background (0) and were not seen at an earlier rank,
    most tokens first (ties by ascending class), until topk are collected."""
    n, c = segs.shape
    order = np.argsort(-segs, axis=1, kind="stable")
    vals = np.take_along_axis(segs, order, axis=1)
    out, used = [], set()
    for k in range(c):
        ids_k = order[:, k]
        rank = []
        for sid in np.unique(ids_k):
            if sid == 0 or int(sid) in used:
                continue
            used.add(int(sid))
            ids = np.where(ids_k == sid)[0]
            rank.append((ids.shape[0], int(sid), ids, float(np.mean(vals[ids, k]))))
        rank.sort(key=lambda item: item[0], reverse=True)      # stable: equal counts stay in ascending class order
        for cnt, sid, ids, score in rank:
            out.append((sid, ids, score))
            if len(out) >= topk:
                return out
    return out


def check_semantic_consistency(q_seg_ids: np.ndarray, frame: dict, start_sid: int, overlap_ratio: float) -> bool:
    ref_sids = np.asarray(frame["keypoint_segs"]) + start_sid
    overlap = np.intersect1d(q_seg_ids, ref_sids)
    n1 = sum(int(np.sum(q_seg_ids == s)) for s in overlap)
    n2 = sum(int(np.sum(ref_sids == s)) for s in overlap)
    with np.errstate(all="ignore"):
        r1 = np.float64(n1) / np.float64(q_seg_ids.shape[0])
        r2 = np.float64(n2) / np.float64(ref_sids.shape[0])
    return bool(min(r1, r2) >= overlap_ratio)


def frame_rows(frame: dict, sid=None) -> np.ndarray:
    """get_keypoints (sid None: every row) / get_keypoints_by_sid (rows with keypoint_segs == sid), original order."""
    n = np.asarray(frame["keypoints"]).shape[0]
    return np.arange(n) if sid is None else np.nonzero(np.asarray(frame["keypoint_segs"]) == sid)[0]


def norm_constants(width, height):
    """normalize_keypoints as the call sites drive it: image_shape = (1, 3, width, height), unpacked as (_, _, height, width)."""
    h_, w_ = float(width), float(height)
    return w_ / 2.0, h_ / 2.0, max(w_, h_) * 0.7


def normalize(kpts: np.ndarray, width, height) -> np.ndarray:
    cx, cy, sc = norm_constants(width, height)
    return ((kpts.astype(np.float32) - np.array([cx, cy], dtype=np.float32)) / np.float32(sc)).astype(np.float32)


def candidates(query: dict, map_: dict, *, seg_k: int, min_kpts: int, semantic_matching: bool = True, overlap_ratio: float = 0.5,
               matcher=None):
    """The loop of MultiMap3D.run for one query, without the pose solver and without its early exit.  -> a list (vote order) of
    dicts: sid (global, vote id - 1), order, semantic_matching, reference_frame (index into map['frames']), q_kpt_ids, ref_rows
    (rows of the frame), data (the matcher's inputs, B = 1 numpy) and, with a matcher, matches0 and the matched_* arrays."""
    frames, start = map_["frames"], int(map_.get("start_sid", 0))
    nq = query["keypoints"].shape[0]
    out = []
    for i, (sid, q_kpt_ids, _) in enumerate(process_segmentations(query["segmentations"], seg_k)):
        sid = sid - 1
        lsid = sid - start
        fid = np.atleast_1d(map_["seg_ref_frame_ids"][lsid])[0].item()
        f = [j for j, fr in enumerate(frames) if fr.get("id", j) == fid][0]
        frame = frames[f]
        if (q_kpt_ids.shape[0] >= min_kpts and semantic_matching
                and check_semantic_consistency(query["seg_ids"], frame, start, overlap_ratio)):
            sem = True
        else:
            q_kpt_ids, sem = np.arange(nq), False
        rows = frame_rows(frame, lsid if (sem and lsid > 0) else None)
        rk = np.asarray(frame["keypoints"], dtype=np.float32)
        data = {"descriptors0": query["descriptors"][q_kpt_ids], "keypoints0": query["keypoints"][q_kpt_ids], "scores0": query["scores"][q_kpt_ids],
                "image_shape0": (1, 3, query["width"], query["height"]),
                "descriptors1": np.asarray(frame["descriptors"], dtype=np.float32)[rows], "keypoints1": rk[rows, :2], "scores1": rk[rows, 2],
                "image_shape1": (1, 3, frame["width"], frame["height"])}
        c = {"sid": sid, "order": i, "semantic_matching": sem, "reference_frame": f, "q_kpt_ids": q_kpt_ids, "ref_rows": rows, "data": data}
        if matcher is not None:
            c["matches0"] = np.asarray(matcher(data))
            c.update(correspondences(c, query, frame))
        out.append(c)
    return out


def correspondences(c: dict, query: dict, frame: dict) -> dict:
    """singlemap3d.py:156-162 from a candidate's matches0."""
    ind = c["matches0"]
    valid = ind >= 0
    rows = c["ref_rows"][ind[valid]]
    return {"matched_keypoints": query["keypoints"][c["q_kpt_ids"]][valid], "matched_keypoint_ids": c["q_kpt_ids"][valid],
            "matched_xyzs": np.asarray(frame["xyzs"], dtype=np.float64)[rows], "matched_point3D_ids": np.asarray(frame["point3D_ids"])[rows],
            "matched_sids": np.asarray(frame["keypoint_segs"])[rows], "matched_ref_keypoints": np.asarray(frame["keypoints"], dtype=np.float32)[rows, :2]}


# ---------------------------------------------------------------- seeded synthetic map and queries
CAMERAS = ((640, 480), (800, 600))


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def make_map(seed: int, n_frames: int = 14, start_sid: int = 0, rows=(600, 1376)) -> dict:
    """n_frames reference frames of rows[0] .. rows[1] keypoints, two camera sizes; frame f carries the labels 2f (45 % of its rows),
    2f + 1 (35 %) and 2f + 2 (the rest; the next frame's first label), shuffled; landmark l's reference frame is frame l // 2.  Frame 0 has rows[1]
    keypoints and frame 1 rows[0]: both ends of the range are always there."""
    rng = np.random.default_rng(seed)
    L = 2 * n_frames
    frames = []
    for f in range(n_frames):
        n = int(rng.integers(rows[0], rows[1] + 1)) if f not in (0, 1) else (rows[1], rows[0])[f]
        w, h = CAMERAS[f % 2]
        a, b = int(0.45 * n), int(0.35 * n)
        segs = np.concatenate([np.full(a, 2 * f), np.full(b, 2 * f + 1), np.full(n - a - b, (2 * f + 2) % L)]).astype(np.int32)
        rng.shuffle(segs)
        kp = np.stack([np.floor(rng.uniform(4, w - 4, n)), np.floor(rng.uniform(4, h - 4, n)), rng.uniform(0, 1, n)], 1).astype(np.float32)
        frames.append({"id": 100 + f, "keypoints": kp, "descriptors": _unit(rng.standard_normal((n, 128))),
                       "xyzs": rng.standard_normal((n, 3)) * 10.0, "point3D_ids": rng.permutation(10 * n)[:n].astype(np.int64) + 100000 * f,
                       "keypoint_segs": segs, "width": w, "height": h})
    return {"frames": frames, "seg_ref_frame_ids": {l: [100 + l // 2, 100 + (l // 2 + 1) % n_frames] for l in range(L)}, "start_sid": start_sid}


def make_query(seed: int, map_: dict, parts, n_pad: int, n_class: int, noise: float = 0.25, camera=(640, 480)) -> dict:
    """A query whose keypoints are noisy twins of reference keypoints.  parts: [(landmark l or None, count)]: `count` keypoints
    twinned from rows of l's reference frame that carry label l (None: background keypoints, fresh descriptors), each with
    segmentation logits peaking at class l + 1 + start_sid (background: class 0).  Descriptor noise: `noise` x the unit norm,
    re-normalised.  The keypoints are shuffled; arrays are padded to n_pad rows (count = the real ones)."""
    rng = np.random.default_rng(seed)
    start = int(map_.get("start_sid", 0))
    w, h = camera
    d, k, cls, twin = [], [], [], []
    for l, cnt in parts:
        if l is None:
            d.append(_unit(rng.standard_normal((cnt, 128))))
            k.append(np.stack([np.floor(rng.uniform(4, w - 4, cnt)), np.floor(rng.uniform(4, h - 4, cnt))], 1))
            cls.append(np.zeros(cnt, dtype=np.int64))
            twin.append(np.full((cnt, 2), -1))
            continue
        fid = map_["seg_ref_frame_ids"][l][0]
        f = [j for j, fr in enumerate(map_["frames"]) if fr["id"] == fid][0]
        fr = map_["frames"][f]
        rows = rng.permutation(np.nonzero(fr["keypoint_segs"] == l)[0])[:cnt]
        assert rows.shape[0] == cnt, (l, cnt, rows.shape)
        d.append(_unit(fr["descriptors"][rows] + noise / np.sqrt(128.0) * rng.standard_normal((cnt, 128))))
        sx, sy = w / fr["width"], h / fr["height"]
        k.append(np.stack([np.clip(np.floor(fr["keypoints"][rows, 0] * sx + rng.integers(-2, 3, cnt)), 0, w - 1),
                           np.clip(np.floor(fr["keypoints"][rows, 1] * sy + rng.integers(-2, 3, cnt)), 0, h - 1)], 1))
        cls.append(np.full(cnt, l + 1 + start, dtype=np.int64))
        twin.append(np.stack([np.full(cnt, f), rows], 1))
    d, k, cls, twin = (np.concatenate(x) if x else np.zeros((0,) + s) for x, s in ((d, (128,)), (k, (2,)), (cls, ()), (twin, (2,))))
    n = d.shape[0]
    perm = rng.permutation(n)
    d, k, cls, twin = d[perm], k[perm], cls[perm].astype(np.int64), twin[perm].astype(np.int64)
    seg = rng.standard_normal((n, n_class)).astype(np.float32)
    seg[np.arange(n), cls] += 8.0
    pad = lambda a: np.concatenate([a, np.zeros((n_pad - n,) + a.shape[1:], dtype=a.dtype)])
    q = {"keypoints": k.astype(np.float32), "scores": rng.uniform(0, 1, n).astype(np.float32), "descriptors": d.astype(np.float32),
         "segmentations": seg, "seg_ids": (np.argmax(seg, 1) - 1).astype(np.int32) if n else np.zeros(0, np.int32), "width": w, "height": h,
         "twin": twin, "count": n}
    q["padded"] = {kk: pad(q[kk]) for kk in ("keypoints", "scores", "descriptors", "segmentations")}
    return q


def batch_features(queries, device):
    """The batched extractor / recogniser outputs of a list of make_query results, on `device`."""
    import torch
    st = lambda key: torch.from_numpy(np.stack([q["padded"][key] for q in queries])).to(device)
    feats = {"keypoints": st("keypoints"), "scores": st("scores"), "descriptors": st("descriptors"),
             "counts": torch.tensor([q["count"] for q in queries], dtype=torch.int32, device=device),
             "image_size": (queries[0]["width"], queries[0]["height"])}
    return feats, st("segmentations")


N_CLASS = 29      # 28 landmarks (make_map's default 14 frames) + background


def oracle_scene(seed: int = 21):
    """Three queries of 512, 300 and 52 keypoints, each twinned from two landmarks whose reference frames are its two candidates
    (semantic matching off: all keypoints of the query against the whole frame, 600 .. 1376 rows)."""
    m = make_map(seed)
    parts = ([(0, 260), (3, 200), (None, 52)], [(8, 150), (11, 100), (None, 50)], [(14, 30), (17, 16), (None, 6)])
    return m, [make_query(seed + 1 + i, m, p, 512, N_CLASS) for i, p in enumerate(parts)]


def plan_scene(seed: int = 31):
    """Six queries padded to 2048 keypoints, seg_k = 5, min_kpts = 32, hitting every branch of the plan:
    0: landmarks 2f, 2f + 1 of a large frame f (semantic on, by-sid reference side), 2f + 2 (enough tokens, consistency fails), a
       stranger with 60 tokens (consistency fails) and one with 20 (< min_kpts);
    1: the same around frame 0: landmark 0 is semantic with in-map id 0 -> the whole frame;
    2, 3: mixtures; 4: background only (the winners come from rank 1); 5: no keypoints at all (fewer than seg_k winners)."""
    m = make_map(seed)
    n = [f["keypoints"].shape[0] for f in m["frames"]]
    f = max(range(2, len(n) - 1), key=lambda j: n[j])
    assert n[f] >= 1200, n
    g = [j for j in range(2, len(n) - 1) if abs(j - f) > 1]
    bg = lambda used: (None, 2048 - used)
    parts = [[(2 * f, 512), (2 * f + 1, 400), (2 * f + 2, 200), (2 * g[0], 60), (2 * g[1], 20), bg(1192)],
             [(0, 512), (1, 400), (2, 200), (2 * g[2], 70), (2 * g[3] + 1, 10), bg(1192)],
             [(2 * g[0], 250), (2 * g[0] + 1, 200), (2 * g[1], 150), (2 * g[2], 100), (2 * g[3], 40), (2 * g[4], 31), bg(771)],
             [(2 * g[1] + 1, 180), (2 * g[2] + 1, 33), (2 * g[3] + 1, 32), (2 * g[4] + 1, 31), bg(276)],
             [bg(0)], []]
    return m, [make_query(seed + 1 + i, m, p, 2048, N_CLASS) for i, p in enumerate(parts)]
