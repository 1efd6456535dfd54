"""Numpy float64 restatement of stage 2b of the triangulation (csrc/triangulate.hip): the rows' adjacency and
every edge's support by third views, in the kernel's order of operations, built on tests/triangulation_ref.py's Track (rays,
centres, depths and residuals) and its scene builders.  The geometry of all (edge, witness) triples is evaluated at once,
elementwise, so every value goes through the same sequence of float64 operations as a lane's.  Also the scenes the CPU and GPU
tests of the stage share."""
from __future__ import annotations

import numpy as np

from tests import triangulation_ref as TR

DEFAULTS = dict(min_support=1, min_tri_angle=1.5, max_reproj_error=4.0)


# ---------------------------------------------------------------- adjacency
def valid_edges(n_rows: int, edges) -> np.ndarray:
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return (e[:, 0] >= 0) & (e[:, 1] >= 0) & (e[:, 0] < n_rows) & (e[:, 1] < n_rows) & (e[:, 0] != e[:, 1])


def adjacency(n_rows: int, edges, frame_off) -> dict:
    """adj_off [n_rows + 1], adj [2 * valid edges] (every row's list ascending, duplicates kept), row_frame [n_rows]."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[valid_edges(n_rows, e)]
    src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    order = np.lexsort((dst, src))
    off = np.zeros(n_rows + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(src, minlength=n_rows)) if n_rows else 0
    row_frame = (np.searchsorted(np.asarray(frame_off), np.arange(n_rows), side="right") - 1).astype(np.int32)
    return {"adj_off": off, "adj": dst[order].astype(np.int32), "row_frame": row_frame}


# ---------------------------------------------------------------- support
def all_rows(scene: dict) -> TR.Track:
    """One Track over every row of the scene: what stage 4 reads of an entry, per row."""
    if "_all_rows" not in scene:
        n = int(scene["frame_off"][-1])
        rows = np.arange(n)
        scene["_all_rows"] = TR.Track(scene, rows, np.searchsorted(np.asarray(scene["frame_off"]), rows, side="right") - 1)
    return scene["_all_rows"]


def _sub(tk: TR.Track, idx) -> TR.Track:
    s = TR.Track.__new__(TR.Track)
    for k in ("rows", "frames", "T", "cam", "obs", "ray", "C"):
        setattr(s, k, getattr(tk, k)[idx])
    return s


def _angle(a, b):
    """TR.angle over columns: a, b [3, K]."""
    c = TR._cross(a, b)
    return np.arctan2(np.sqrt(TR._dot(c, c)), TR._dot(a, b))


def midpoint(C1, d1, C2, d2):
    """Stage 4's hypothesis of two rays, over columns [3, K]."""
    w = C1 - C2
    a, b, c, d, e = TR._dot(d1, d1), TR._dot(d1, d2), TR._dot(d2, d2), TR._dot(d1, w), TR._dot(d2, w)
    den = a * c - b * b
    with np.errstate(all="ignore"):
        s, u = (b * e - c * d) / den, (a * e - b * d) / den
    return 0.5 * ((C1 + s * d1) + (C2 + u * d2))


def witnesses(adj: dict, n_rows: int, u: int, v: int) -> list:
    """As the lanes meet them: adj(u) then adj(v), an element equal to its predecessor or (of adj(v)) found in adj(u) skipped."""
    off, a, rf = adj["adj_off"], adj["adj"], adj["row_frame"]
    lu, lv = a[off[u]:off[u + 1]], a[off[v]:off[v + 1]]
    out = []
    for k, w in enumerate(lu.tolist()):
        if k > 0 and lu[k - 1] == w:
            continue
        out.append(w)
    for k, w in enumerate(lv.tolist()):
        if k > 0 and lv[k - 1] == w:
            continue
        p = int(np.searchsorted(lu, w, side="left"))
        if p < len(lu) and lu[p] == w:
            continue
        out.append(w)
    return [w for w in out if 0 <= w < n_rows and w != u and w != v and rf[w] != rf[u] and rf[w] != rf[v]]


def support(scene: dict, edges, min_support: int = 1, min_tri_angle: float = 1.5, max_reproj_error: float = 4.0) -> dict:
    """-> support int32 [n], keep, edges (filtered) and ``trace``: per (edge, witness) triple ``edge``, ``rows`` (u, v, w),
    ``angles`` (u, v), (u, w), (v, w) in radians, ``pick``, ``reached`` (the largest angle is min_tri_angle at least), ``err`` (the
    three reprojection errors in pixels) and ``confirm``; ``adj``: the adjacency."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    n_rows = int(scene["frame_off"][-1])
    adj = adjacency(n_rows, e, scene["frame_off"])
    rf = adj["row_frame"]
    ok = valid_edges(n_rows, e)
    tri = []
    for i in np.nonzero(ok)[0].tolist():
        u, v = int(e[i, 0]), int(e[i, 1])
        if rf[u] == rf[v]:
            continue
        tri.extend((i, u, v, w) for w in witnesses(adj, n_rows, u, v))
    tri = np.array(tri, dtype=np.int64).reshape(-1, 4)
    tk = all_rows(scene)
    min_angle, thr2 = float(np.deg2rad(min_tri_angle)), max_reproj_error * max_reproj_error
    U, V, W = (_sub(tk, tri[:, k]) for k in (1, 2, 3))
    du, dv, dw, Cu, Cv, Cw = U.ray.T, V.ray.T, W.ray.T, U.C.T, V.C.T, W.C.T
    ang = np.stack([_angle(du, dv), _angle(du, dw), _angle(dv, dw)], 1).reshape(-1, 3)
    pick, best = np.zeros(len(tri), dtype=np.int64), ang[:, 0].copy()
    for k in (1, 2):      # the first of the largest
        better = ang[:, k] > best
        pick[better], best[better] = k, ang[better, k]
    reached = best >= min_angle
    X = np.where(pick == 0, midpoint(Cu, du, Cv, dv), np.where(pick == 1, midpoint(Cu, du, Cw, dw), midpoint(Cv, dv, Cw, dw)))
    inl, err = [], []
    for t in (U, V, W):
        m, e2 = t.inliers(X, thr2)
        inl.append(m)
        with np.errstate(all="ignore"):
            err.append(np.sqrt(e2))
    confirm = reached & inl[0] & inl[1] & inl[2]
    sup = np.bincount(tri[confirm, 0], minlength=len(e)).astype(np.int32)
    keep = sup >= min_support
    return {"support": sup, "keep": keep, "edges": np.where(keep[:, None], e, -1).astype(np.int32), "adj": adj,
            "trace": {"edge": tri[:, 0], "rows": tri[:, 1:], "angles": ang, "pick": pick, "reached": reached,
                      "err": np.stack(err, 1).reshape(-1, 3), "confirm": confirm}}


def run(scene: dict, min_support: int = 0, **params) -> dict:
    """TR.run with stage 2b between verification and the components -> TR.run's dict plus ``support`` and ``edges``."""
    p = {**TR.DEFAULTS, **params}
    use = TR.unique_pairs(scene["pairs"])
    v = TR.verify(scene["norm0"], scene["frame_off"], scene["table"], scene["pairs"][use], [scene["matches"][i] for i in use], p["max_error"])
    sup = support(scene, v["edges"], min_support, p["min_tri_angle"], p["max_reproj_error"]) if min_support > 0 else None
    edges = v["edges"] if sup is None else sup["edges"]
    label = TR.components(int(scene["frame_off"][-1]), edges)
    trk = TR.tracks(label, scene["frame_off"])
    tri = TR.triangulate(scene, trk, trials=p["trials"], seed=p["seed"], min_tri_angle=p["min_tri_angle"], max_reproj_error=p["max_reproj_error"])
    return {"pair_index": use, "verify": v, "support": sup, "edges": edges, "label": label, "tracks": trk, "tri": tri}


def track_conflicts(trk: dict) -> np.ndarray:
    """Per track the number of frames that hold more than one entry, by a loop."""
    out = []
    for a, b in zip(trk["trk_off"][:-1], trk["trk_off"][1:]):
        f = np.asarray(trk["trk_frame"][a:b]).tolist()
        out.append(sum(1 for x in set(f) if f.count(x) > 1))
    return np.array(out, dtype=np.int64)


# ---------------------------------------------------------------- scenes
_scenes: dict = {}


def _split(s: dict) -> list:
    return [[tuple(k) for k in s["keypoints"][a:b].tolist()] for a, b in zip(s["frame_off"][:-1], s["frame_off"][1:])]


def glued_scene(noise: float = TR.NOISE, seed: int = 21) -> dict:
    """Six frames on an arc.  Point 0 is seen in frames 0-3, point 1 in frames 2-5, all pairs of each matched.  Point 1 lies in the
    epipolar plane of point 0's keypoint in frame 0 and frame 4 (on frame 4's ray to a place Y further out on that keypoint's
    ray), so its keypoint in frame 4 is on that keypoint's epipolar line: the one wrong match (``bridge``, rows) of pair (0, 4)
    passes verification and glues the two tracks into one component.  The two rays of the bridge meet at Y, which nothing else
    sees; a bridge whose rays met at one of the two points would be a true observation of that point as far as geometry goes."""
    key = ("glued", noise, seed)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.RandomState(seed)
    F = 6
    ang = np.deg2rad(np.linspace(-30.0, 30.0, F))
    centres = [np.array([8.0 * np.sin(a), 0.3 * np.cos(3 * a), -8.0 * np.cos(a)]) for a in ang]
    s = TR._base([TR.CAMERAS[f % 5] for f in range(F)], centres, [np.zeros(3)] * F)
    A = np.array([0.4, -0.3, 0.5])
    px, z = TR.project(s, 0, A)
    kA0 = (px[0] - 0.5 + rng.uniform(-noise, noise, size=2)).astype(np.float32)
    n0 = TR.normalize(kA0[None], [0, 1], s["cam_model"][0:1], s["cam_params"][0:1], 0.5)[0]
    ray0 = s["table"][0, :9].reshape(3, 3).T @ np.array([n0[0], n0[1], 1.0])
    Y = s["table"][0, 12:15] + 1.5 * float(z[0]) * ray0      # where the bridge's two rays meet: no point of the scene
    xyz = np.stack([A, s["table"][4, 12:15] + 0.7 * (Y - s["table"][4, 12:15])])
    seen = {0: (0, 1, 2, 3), 1: (2, 3, 4, 5)}
    kps, where = [[] for _ in range(F)], {}
    for f in range(F):
        for p in rng.permutation(2).tolist():
            if f in seen[p]:
                px, z = TR.project(s, f, xyz[p])
                assert z[0] > 0.5 and 8.0 <= px[0, 0] < TR.WIDTH - 8.0 and 8.0 <= px[0, 1] < TR.HEIGHT - 8.0
                kps[f].append(tuple(kA0.tolist()) if (f, p) == (0, 0) else tuple(px[0] - 0.5 + rng.uniform(-noise, noise, size=2)))
                where[(f, p)] = len(kps[f]) - 1
    pairs = [(a, b) for a in range(F) for b in range(a + 1, F)]
    matches = [[(where[(a, p)], where[(b, p)]) for p in (0, 1) if a in seen[p] and b in seen[p]] for a, b in pairs]
    matches[pairs.index((0, 4))].append((where[(0, 0)], where[(4, 1)]))
    s.update(pairs=pairs, matches=matches, xyz=xyz, where=where, seen=seen, noise=noise)
    s = TR._finish(s, kps)
    s["bridge"] = (int(s["frame_off"][0]) + where[(0, 0)], int(s["frame_off"][4]) + where[(4, 1)])
    _scenes[key] = s
    return s


STAR_FRAMES = 70
STAR_LENGTHS = {2, 3, 63, 64, 65, 66, 67, 130}      # deg(u) + deg(v) of the tested edges, see star_scene


def star_scene(seed: int = 5) -> dict:
    """TR.ring_scene with four points seen in all 70 frames, two far points added (``lp`` in frames 0, 1 and 5; ``lq`` in frames
    0, 1 and 2: at a depth of about 90 neighbouring frames see them under less than 1.5 degrees) and an edge list of its own
    (``edges``, rows, shuffled) instead of matches.  ``tested``: name -> (u, v) of the edges the tests look at.

    deg(u) + deg(v) is the length of the list a wave walks.  An edge that counts adds one to each end, so the smallest length is
    2: the lengths here are 2 and 3 (0 and 1 neighbours besides the edge itself), 63 to 67 (the strides around one wave, and 63,
    64, 65 neighbours besides), 130, and 200 and more at the hub, whose row has degree 200; the edges that do not count have
    length 0."""
    key = ("star", seed)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.RandomState(seed)
    s0 = TR.ring_scene(lengths=(STAR_FRAMES,) * 4, n_frames=STAR_FRAMES, seed=seed)
    s = {k: s0[k] for k in ("cameras", "cam_model", "cam_params", "qvec", "tvec", "table", "n_frames")}
    kps, where = _split(s0), dict(s0["where"])
    far = {"lp": (np.array([0.3, 0.2, 80.0]), (0, 1, 5)), "lq": (np.array([-0.2, 0.1, 80.0]), (0, 1, 2))}
    for name, (X, frames) in far.items():
        for f in frames:
            px, z = TR.project(s, f, X)
            assert z[0] > 0 and 8.0 <= px[0, 0] < TR.WIDTH - 8.0 and 8.0 <= px[0, 1] < TR.HEIGHT - 8.0, (name, f, px)
            kps[f].append(tuple(px[0] - 0.5 + rng.uniform(-s0["noise"], s0["noise"], size=2)))
            where[(f, name)] = len(kps[f]) - 1
    s.update(pairs=[], matches=[], where=where, xyz=s0["xyz"], far={k: v[0] for k, v in far.items()}, noise=s0["noise"])
    s = TR._finish(s, kps)
    n_rows = int(s["frame_off"][-1])
    R = lambda f, p: int(s["frame_off"][f]) + where[(f, p)]
    hub = R(0, 0)      # 69 true edges and 131 wrong ones: degree 200
    E = [(hub, R(f, 0)) for f in range(1, 70)] + [(hub, R(f, 1)) for f in range(1, 70)] + [(hub, R(f, 2)) for f in range(1, 63)]
    l = lambda f: R(f, 3)
    c1 = l(5)          # a star over point 3: 61 leaves and one of its edges given twice, the second time reversed: degree 62
    E += [(l(0), l(1)), (l(2), l(3)), (l(3), l(4))]
    E += [(c1, l(f)) for f in range(6, 67)] + [(l(20), c1)]
    E += [(l(6), l(7))]                                                    # a triangle with c1
    E += [(l(8), l(9)), (l(8), l(10))]
    E += [(l(11), l(f)) for f in (12, 13, 14)] + [(l(15), l(f)) for f in (16, 17, 18, 19)]
    E += [(l(31), R(5, 1))]                                                # a neighbour of l(31) in c1's frame
    c2, c3 = R(0, 1), R(69, 2)                                             # two stars of 64 leaves, joined by a wrong edge
    E += [(c2, R(f, 1)) for f in range(1, 65)] + [(c3, R(f, 2)) for f in range(0, 64)] + [(c2, c3)]
    E += [(R(68, 1), R(68, 2))]                                            # both rows in frame 68
    E += [(-1, -1), (n_rows, 0), (0, n_rows), (7, 7), (-1, 3)]
    E += [(R(0, "lp"), R(1, "lp")), (R(0, "lp"), R(5, "lp"))]
    E += [(R(0, "lq"), R(1, "lq")), (R(1, "lq"), R(2, "lq")), (R(0, "lq"), R(2, "lq"))]
    s["edges"] = np.array(E, dtype=np.int64)[rng.permutation(len(E))]
    s["tested"] = {"hub": (hub, R(1, 0)), "len2": (l(0), l(1)), "len3": (l(2), l(3)), "len63": (c1, l(30)), "len64": (c1, l(6)),
                   "len65": (c1, l(8)), "len66": (c1, l(11)), "len67": (c1, l(15)), "len130": (c2, c3), "duplicate": (c1, l(20)),
                   "duplicate_reversed": (l(20), c1), "triangle": (c1, l(7)), "same_frame_neighbour": (c1, l(31)),
                   "same_frame_edge": (R(68, 1), R(68, 2)), "low_parallax": (R(0, "lp"), R(1, "lp")),
                   "low_parallax_triple": (R(0, "lq"), R(1, "lq")), "none": (-1, -1), "past_the_end": (n_rows, 0), "loop": (7, 7)}
    s["hub"], s["lonely"] = hub, l(69)
    _scenes[key] = s
    return s


def edge_index(scene: dict, uv) -> int:
    return int(np.nonzero((scene["edges"] == np.asarray(uv)).all(1))[0][0])


def sweep_scene(p: float, seed: int, n_points: int = 200, n_frames: int = 20) -> dict:
    """The geometric simulation: ``n_frames`` frames on a ring, ``n_points`` points each seen in 4 to 9 consecutive frames (the ring
    closes), pairs up to 3 frames apart, keypoint noise TR.NOISE, every true match present; wrong matches, a share ``p`` of the
    true ones, drawn among the keypoint pairs of two different points whose epipolar errors are both below 3 px, so that every
    one of them passes verification.  ``owner`` [n_rows]: each row's point."""
    key = ("sweep", p, seed, n_points, n_frames)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.RandomState(seed)
    F = n_frames
    ang = np.linspace(0.0, 2.0 * np.pi, F, endpoint=False)
    centres = [np.array([9.0 * np.sin(a), 0.4 * np.sin(5 * a), -9.0 * np.cos(a)]) for a in ang]
    s = TR._base([TR.CAMERAS[f % 5] for f in range(F)], centres, [np.zeros(3)] * F)
    xyz = rng.uniform(-1.0, 1.0, size=(n_points, 3))
    start, length = rng.randint(F, size=n_points), rng.randint(4, 10, size=n_points)
    kps, where, owner = [[] for _ in range(F)], {}, []
    for f in range(F):
        px, z = TR.project(s, f, xyz)
        for q in rng.permutation(n_points).tolist():
            if (f - start[q]) % F < length[q]:
                assert z[q] > 0 and 0 <= px[q, 0] < TR.WIDTH and 0 <= px[q, 1] < TR.HEIGHT
                kps[f].append(tuple(px[q] - 0.5 + rng.uniform(-TR.NOISE, TR.NOISE, size=2)))
                where[(f, q)] = len(kps[f]) - 1
                owner.append(q)
    pairs = [(f, (f + d) % F) for d in (1, 2, 3) for f in range(F)]
    matches = [[(where[(a, q)], where[(b, q)]) for q in range(n_points) if (a, q) in where and (b, q) in where] for a, b in pairs]
    s.update(pairs=pairs, matches=[[] for _ in pairs], xyz=xyz, where=where, noise=TR.NOISE)
    s = TR._finish(s, kps)
    owner = np.array(owner, dtype=np.int64)
    n_true = sum(len(m) for m in matches)
    cand = []
    for k, (a, b) in enumerate(pairs):
        ra, rb = np.arange(s["frame_off"][a], s["frame_off"][a + 1]), np.arange(s["frame_off"][b], s["frame_off"][b + 1])
        I, J = (x.ravel() for x in np.meshgrid(ra, rb, indexing="ij"))
        e0, e1 = TR.epipolar_errors(TR.essential(s["table"][a], s["table"][b]), s["norm0"][I], s["norm0"][J])
        ok = (e0 * s["table"][a, 15] < 3.0) & (e1 * s["table"][b, 15] < 3.0) & (owner[I] != owner[J])
        cand.extend((k, int(i - ra[0]), int(j - rb[0])) for i, j in zip(I[ok].tolist(), J[ok].tolist()))
    n_wrong = int(round(p * n_true))
    for c in rng.permutation(len(cand))[:n_wrong].tolist():
        matches[cand[c][0]].append(cand[c][1:])
    s["matches"] = [np.asarray(m, dtype=np.int64).reshape(-1, 2)[rng.permutation(len(m))] for m in matches]
    s.update(owner=owner, n_true=n_true, n_wrong=n_wrong)
    _scenes[key] = s
    return s
