"""Numpy restatement of the reference's candidate loop over SEVERAL maps, for the tests of pram_amd.localization.multimap.

Written from MultiMap3D.initialize_map / run (localization/multimap3d.py:58-93, 110-145): sid_scene_name[sid] names the sub-map
that owns a voted landmark, scene_name_start_sid[name] its first global id, and check_semantic_consistency /
localize_with_ref_frame then run inside that sub-map with the in-map id.  ``maps`` is a list of cand_ref maps (dict(frames,
seg_ref_frame_ids, start_sid)); the owner of a global id is the map whose range [start_sid, start_sid + n_landmarks) holds it.
Refinement and tracking inside the owning map are refine_ref / projref_ref / track_ref applied to that map.

Also the seeded scenes the CPU and GPU tests share (two_maps, mixed_query, pinned_cases, twin_maps)."""
from __future__ import annotations

import numpy as np

from tests import cand_ref as CR
from tests import refine_ref as RR


def n_landmarks(map_: dict) -> int:
    s = map_["seg_ref_frame_ids"]
    return (max((int(k) for k in s), default=-1) + 1) if isinstance(s, dict) else len(s)


def owner(maps, gsid: int):
    """-> (map index, in-map id) of global landmark gsid, or None where no map's range holds it (the reference raises there)."""
    for m, mp in enumerate(maps):
        l = gsid - int(mp.get("start_sid", 0))
        if 0 <= l < n_landmarks(mp):
            return m, l
    return None


def reference_frame(map_: dict, lsid: int):
    """Index into map_['frames'] of the landmark's reference frame (entry [0] of its list), None without one."""
    s = map_["seg_ref_frame_ids"]
    v = s.get(lsid) if isinstance(s, dict) else s[lsid]
    v = np.atleast_1d(np.asarray(v if v is not None else []))
    if v.size == 0:
        return None
    return [j for j, fr in enumerate(map_["frames"]) if fr.get("id", j) == v[0].item()][0]


def decide(seg_ids: np.ndarray, n_tokens: int, maps, gsid: int, *, min_kpts: int, semantic_matching: bool = True, overlap_ratio: float = 0.5):
    """multimap3d.py:119-139 for one voted landmark.  -> None (nobody's landmark, or no reference frame) or dict(map, lsid, frame
    (in-map index), semantic_matching, by_sid)."""
    own = owner(maps, gsid)
    if own is None:
        return None
    m, lsid = own
    f = reference_frame(maps[m], lsid)
    if f is None:
        return None
    sem = bool(n_tokens >= min_kpts and semantic_matching
               and CR.check_semantic_consistency(seg_ids, maps[m]["frames"][f], int(maps[m].get("start_sid", 0)), overlap_ratio))
    return {"map": m, "lsid": lsid, "frame": f, "semantic_matching": sem, "by_sid": sem and lsid > 0}


def candidates(query: dict, maps, *, seg_k: int, min_kpts: int, semantic_matching: bool = True, overlap_ratio: float = 0.5, matcher=None):
    """cand_ref.candidates with the map chosen per candidate.  -> a list (vote order) of dicts: cand_ref's keys plus map (index
    into maps; None for a landmark nobody owns, which comes back as the empty candidate), lsid (in-map id) and store_frame (frame
    index counted over all maps); reference_frame stays the index into the owning map's frames."""
    nq = query["keypoints"].shape[0]
    frame_off = np.concatenate([[0], np.cumsum([len(mp["frames"]) for mp in maps])])
    out = []
    for i, (sid, q_kpt_ids, _) in enumerate(CR.process_segmentations(query["segmentations"], seg_k)):
        sid = sid - 1
        d = decide(query["seg_ids"], q_kpt_ids.shape[0], maps, sid, min_kpts=min_kpts, semantic_matching=semantic_matching, overlap_ratio=overlap_ratio)
        if d is None:
            out.append({"sid": sid, "order": i, "semantic_matching": False, "map": None, "lsid": None, "reference_frame": None, "store_frame": -1,
                        "q_kpt_ids": np.zeros(0, dtype=np.int64), "ref_rows": np.zeros(0, dtype=np.int64), "data": None})
            continue
        frame = maps[d["map"]]["frames"][d["frame"]]
        if not d["semantic_matching"]:
            q_kpt_ids = np.arange(nq)
        rows = CR.frame_rows(frame, d["lsid"] if d["by_sid"] else None)
        rk = np.asarray(frame["keypoints"], dtype=np.float32)
        data = {"descriptors0": query["descriptors"][q_kpt_ids], "keypoints0": query["keypoints"][q_kpt_ids], "scores0": query["scores"][q_kpt_ids],
                "image_shape0": (1, 3, query["width"], query["height"]),
                "descriptors1": np.asarray(frame["descriptors"], dtype=np.float32)[rows], "keypoints1": rk[rows, :2], "scores1": rk[rows, 2],
                "image_shape1": (1, 3, frame["width"], frame["height"])}
        c = {"sid": sid, "order": i, "semantic_matching": d["semantic_matching"], "map": d["map"], "lsid": d["lsid"], "reference_frame": d["frame"],
             "store_frame": int(frame_off[d["map"]]) + d["frame"], "q_kpt_ids": q_kpt_ids, "ref_rows": rows, "data": data}
        if matcher is not None:
            c["matches0"] = np.asarray(matcher(data))
            c.update(CR.correspondences(c, query, frame))
        out.append(c)
    return out


# ---------------------------------------------------------------- seeded scenes
TWO_NAMES = ("office", "stairs")
TWO_N_CLASS = 19      # background + 10 landmarks of the first map + 8 of the second
TWO_SEG_K, TWO_MIN_KPTS, TWO_N_PAD = 6, 8, 128


def two_maps():
    """Two small maps in one numbering: 5 frames / landmarks 0 .. 9 and 4 frames / landmarks 10 .. 17, 40 .. 90 rows a frame.  Both
    number their frames from 100 and draw their point ids from the same small range: raw ids occur in both."""
    a = CR.make_map(7, n_frames=5, start_sid=0, rows=(40, 90))
    b = CR.make_map(8, n_frames=4, start_sid=10, rows=(40, 90))
    ids = [np.concatenate([f["point3D_ids"] for f in m["frames"]]) for m in (a, b)]
    assert np.intersect1d(*ids).size > 0 and a["frames"][0]["id"] == b["frames"][0]["id"] == 100
    return [a, b]


def _join(seed: int, maps, parts_per_map, n_background: int, n_pad: int = TWO_N_PAD, n_class: int = TWO_N_CLASS) -> dict:
    """cand_ref.make_query on each map with that map's parts, the real rows joined (map order, then background) and padded."""
    qs = [CR.make_query(seed + 10 * m, mp, parts, n_pad, n_class) for m, (mp, parts) in enumerate(zip(maps, parts_per_map)) if parts]
    qs.append(CR.make_query(seed + 99, maps[0], [(None, n_background)], n_pad, n_class))
    keys = ("keypoints", "scores", "descriptors", "segmentations", "seg_ids")
    q = {k: np.concatenate([x[k][:x["count"]] for x in qs]) for k in keys}
    q["count"] = n = q["keypoints"].shape[0]
    q["width"], q["height"] = qs[0]["width"], qs[0]["height"]
    q["padded"] = {k: np.concatenate([q[k], np.zeros((n_pad - n,) + q[k].shape[1:], dtype=q[k].dtype)]) for k in keys[:4]}
    return q


def mixed_query(maps=None) -> dict:
    """One query twinned from three landmarks of each map of two_maps(), 16 rows a landmark at the most, with token counts 16, 15,
    14, 13, 12, 11 falling to the maps in turn: its six candidates alternate between the maps, the second being in-map id 0 of
    the second map."""
    maps = two_maps() if maps is None else maps
    return _join(41, maps, ([(0, 16), (1, 14), (4, 12)], [(0, 15), (1, 13), (5, 11)]), 7)


def pinned_cases(maps=None):
    """mixed_query plus one query per map whose keypoints sit on the two landmarks of one reference frame (semantic matching
    holds: in-map ids 0, whole frame, and 1, by landmark)."""
    maps = two_maps() if maps is None else maps
    return [mixed_query(maps), _join(42, maps, ([(0, 16), (1, 14)], []), 6), _join(43, maps, ([], [(0, 16), (1, 14)]), 5)]


def real(q: dict) -> dict:
    """the query as the restatement takes it: the real keypoints only"""
    return {k: (v[:q["count"]] if isinstance(v, np.ndarray) else v) for k, v in q.items() if k != "padded"}


TWIN_NAMES = ("a", "b")
TWIN_START = (0, 11)
TWIN_N_CLASS = 23     # background + covisible_scene's 11 landmarks, twice
_FILL = -100.0        # a class column no token ever ranks above a real one


def shift_logits(seg: np.ndarray, first: int, n_class: int = TWIN_N_CLASS) -> np.ndarray:
    """[n, 1 + L] logits -> [n, n_class] with the L landmark columns at classes first + 1 .. first + L, the others filled low."""
    out = np.full((seg.shape[0], n_class), _FILL, dtype=np.float32)
    out[:, 0] = seg[:, 0]
    out[:, 1 + first:first + seg.shape[1]] = seg[:, 1:]
    return out


def twin_queries(queries, n_pad: int, starts=TWIN_START, n_class: int = TWIN_N_CLASS):
    """Every query once per map: as generated (landmark columns at the first map's classes), then with them moved to the next
    map's classes.  Query i of map m sits at m * len(queries) + i."""
    out = []
    for first in starts:
        for q in queries:
            t = dict(q)
            n = q["count"]
            t["segmentations"] = shift_logits(q["segmentations"], first, n_class)
            t["seg_ids"] = np.where(q["seg_ids"] >= 0, q["seg_ids"] + first, q["seg_ids"]).astype(np.int32)
            assert np.array_equal(t["seg_ids"], (np.argmax(t["segmentations"], 1) - 1).astype(np.int32) if n else t["seg_ids"])
            t["padded"] = dict(q["padded"], segmentations=np.concatenate([t["segmentations"], np.zeros((n_pad - n, n_class), dtype=np.float32)]))
            out.append(t)
    return out


def twin_of(map_: dict, start_sid: int) -> dict:
    return dict(map_, start_sid=start_sid)


def twin_maps(seed: int = 7):
    """refine_ref.covisible_scene's map twice, as 'a' (landmarks 0 .. 10) and 'b' (11 .. 21): the same frames, frame ids and point
    ids in both.  -> (maps, queries (twin_queries of the scene's five, padded to 192), planted (per query, both halves))."""
    m, qs, planted = RR.covisible_scene(seed)
    assert n_landmarks(m) == TWIN_START[1] and RR.N_CLASS == TWIN_START[1] + 1
    return [twin_of(m, s) for s in TWIN_START], twin_queries(qs, RR.N_PAD), planted + planted
