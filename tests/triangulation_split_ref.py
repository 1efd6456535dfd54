"""Numpy restatement of the triangulation's further rounds (``split_rounds``; pram_tri_split of csrc/triangulate.hip, DESIGN.md
4.21): the restated stages 3 and 4 of tests/triangulation_ref.py (components, tracks, triangulate) composed round after round,
with the marking of the rows and the filter of the edges between them written as loops.  Also the scenes the CPU and GPU tests of
the rounds share, and which runs the GPU test makes (GPU_RUNS)."""
from __future__ import annotations

import numpy as np

from tests import triangulation_ref as TR
from tests import triangulation_support_ref as SR

FREE, TAKEN, DEAD = 0, 1, 2      # PRAM_TRI_ROW_*
NEAR = 0.01                      # a planted point counts as found when an accepted point lies within 1 cm of it


# ---------------------------------------------------------------- marking and filtering
def mark(state: np.ndarray, trk: dict, tri: dict) -> None:
    """Every entry of the round's table onto its row of ``state`` (uint8 [n_rows], in place)."""
    n, E = len(state), len(trk["trk_row"])
    clamp = lambda o: min(max(int(o), 0), E)
    for t in range(len(trk["trk_off"]) - 1):
        beg = clamp(trk["trk_off"][t])
        end = max(clamp(trk["trk_off"][t + 1]), beg)
        for e in range(beg, end):
            r = int(trk["trk_row"][e])
            if r < 0 or r >= n:
                continue
            if not tri["accept"][t]:
                state[r] = DEAD
            elif tri["entry_keep"][e]:
                state[r] = TAKEN
            else:
                state[r] = FREE


def filter_edges(state: np.ndarray, edges) -> tuple:
    """-> (edges int32 [n, 2] with (-1, -1) where an end is out of range or not FREE, the number of edges that stay)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    out, n_live, n = np.full(e.shape, -1, dtype=np.int32), 0, len(state)
    for i, (u, v) in enumerate(e.tolist()):
        if 0 <= u < n and 0 <= v < n and state[u] == FREE and state[v] == FREE:
            out[i] = (u, v)
            n_live += 1
    return out, n_live


def split(n_rows: int, trk: dict, tri: dict, edges, state=None) -> dict:
    """What ops.tri_split computes: state None starts from all DEAD."""
    state = np.full(n_rows, DEAD, dtype=np.uint8) if state is None else np.array(state, dtype=np.uint8)
    mark(state, trk, tri)
    e, n_live = filter_edges(state, edges)
    return {"state": state, "edges": e, "n_live": n_live}


# ---------------------------------------------------------------- the rounds
_TRI = ("trials", "seed", "min_tri_angle", "max_reproj_error")


def rounds(scene: dict, edges, split_rounds: int, first: dict = None, **params) -> list:
    """edges: the rows round 0's tracks are built from -> one dict per round begun.  Round 0 and every further round that found a
    track hold ``label``, ``tracks`` and ``tri``; every further round holds ``state`` (after marking), ``edges`` (filtered) and
    ``n_live``, and ``tracks`` is None in one that stopped for want of an edge or a track.  first: round 0 when it is at hand."""
    p = {k: {**TR.DEFAULTS, **params}[k] for k in _TRI}
    n, fo = int(scene["frame_off"][-1]), scene["frame_off"]
    if first is None:
        label = TR.components(n, edges)
        trk = TR.tracks(label, fo)
        first = {"label": label, "tracks": trk, "tri": TR.triangulate(scene, trk, **p)}
    out, state = [first], None
    for _ in range(split_rounds):
        s = split(n, out[-1]["tracks"], out[-1]["tri"], edges, state)
        state = s["state"]
        rec = {**s, "label": None, "tracks": None, "tri": None}
        out.append(rec)
        if s["n_live"] == 0:
            break
        label = TR.components(n, s["edges"])
        trk = TR.tracks(label, fo)
        if len(trk["trk_label"]) == 0:
            break
        rec.update(label=label, tracks=trk, tri=TR.triangulate(scene, trk, **p))
    return out


_runs: dict = {}


def run(scene: dict, min_support: int = 0, split_rounds: int = 0, **params) -> dict:
    """SR.run (verification, stage 2b, round 0) followed by the further rounds -> SR.run's dict plus ``rounds``."""
    key = (id(scene), min_support, split_rounds, tuple(sorted(params.items())))
    if key not in _runs:
        base = SR.run(scene, min_support, **params)
        base["rounds"] = rounds(scene, base["edges"], split_rounds, first={k: base[k] for k in ("label", "tracks", "tri")}, **params)
        _runs[key] = base
    return _runs[key]


def complete(r: dict) -> list:
    """The rounds that reached stage 4."""
    return [x for x in r["rounds"] if x["tracks"] is not None]


def points(r: dict) -> tuple:
    """(xyz [P, 3], round [P]) of the accepted tracks, round 0's first, each round's in track order."""
    done = complete(r)
    xyz = np.concatenate([x["tri"]["xyz"][x["tri"]["accept"]].reshape(-1, 3) for x in done])
    return xyz, np.repeat(np.arange(len(done)), [int(x["tri"]["accept"].sum()) for x in done])


def distinct_found(scene: dict, xyz) -> set:
    """The planted points that have an accepted point within NEAR."""
    xyz = np.asarray(xyz).reshape(-1, 3)
    if not len(xyz):
        return set()
    d = np.linalg.norm(xyz[:, None, :] - scene["xyz"][None, :, :], axis=2)
    return set(d.argmin(1)[d.min(1) <= NEAR].tolist())


# ---------------------------------------------------------------- scenes
_scenes: dict = {}
ARC_FRAMES = 8


def arc_scene(name: str, seen: dict, bridges=(), fixed: dict = None, noise: float = TR.NOISE, seed: int = 31) -> dict:
    """Eight frames on an arc, built like SR.glued_scene.  seen: point -> the frames that see it, all pairs of them matched.
    Point 0 is planted; fixed: further planted points.  bridges: (p, fp, q, fq, depth): point q is placed on frame fq's ray to a
    place Y on the ray of p's stored keypoint in frame fp, ``depth`` times as far out as p, so q's keypoint in frame fq lies on that
    keypoint's epipolar line and the wrong match between the two (``bridge_rows``) passes verification; fq sees no p and fp no
    q."""
    key = (name, noise, seed)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.RandomState(seed)
    F = ARC_FRAMES
    ang = np.deg2rad(np.linspace(-35.0, 35.0, F))
    centres = [np.array([8.0 * np.sin(a), 0.3 * np.cos(3 * a), -8.0 * np.cos(a)]) for a in ang]
    s = TR._base([TR.CAMERAS[f % 5] for f in range(F)], centres, [np.zeros(3)] * F)
    xyz = {0: np.array([0.4, -0.3, 0.5]), **{p: np.asarray(x, dtype=np.float64) for p, x in (fixed or {}).items()}}
    stored = {}      # (frame, point) -> the stored keypoint

    def observe(p):
        for f in seen[p]:
            px, z = TR.project(s, f, xyz[p])
            assert z[0] > 0.5 and 8.0 <= px[0, 0] < TR.WIDTH - 8.0 and 8.0 <= px[0, 1] < TR.HEIGHT - 8.0, (name, p, f, px)
            stored[(f, p)] = (px[0] - 0.5 + rng.uniform(-noise, noise, size=2)).astype(np.float32)

    for p in sorted(xyz):
        observe(p)
    for p, fp, q, fq, depth in bridges:
        assert fp in seen[p] and fq in seen[q] and fq not in seen[p] and fp not in seen[q] and q not in xyz
        n0 = TR.normalize(stored[(fp, p)][None], [0, 1], s["cam_model"][fp:fp + 1], s["cam_params"][fp:fp + 1], 0.5)[0]
        ray = s["table"][fp, :9].reshape(3, 3).T @ np.array([n0[0], n0[1], 1.0])
        Y = s["table"][fp, 12:15] + depth * float(TR.project(s, fp, xyz[p])[1][0]) * ray
        xyz[q] = s["table"][fq, 12:15] + 0.7 * (Y - s["table"][fq, 12:15])
        observe(q)
    kps, where = [[] for _ in range(F)], {}
    for f in range(F):
        here = [p for p in sorted(xyz) if f in seen[p]]
        for p in [here[i] for i in rng.permutation(len(here)).tolist()]:
            kps[f].append(tuple(stored[(f, p)].tolist()))
            where[(f, p)] = len(kps[f]) - 1
    pairs = [(a, b) for a in range(F) for b in range(a + 1, F)]
    matches = [[(where[(a, p)], where[(b, p)]) for p in sorted(xyz) if a in seen[p] and b in seen[p]] for a, b in pairs]
    for p, fp, q, fq, _ in bridges:
        a, b = (fp, fq) if fp < fq else (fq, fp)
        matches[pairs.index((a, b))].append((where[(a, p if a == fp else q)], where[(b, q if b == fq else p)]))
    s.update(pairs=pairs, matches=matches, xyz=np.stack([xyz[p] for p in sorted(xyz)]), where=where, seen=dict(seen), noise=noise)
    s = TR._finish(s, kps)
    row = lambda f, p: int(s["frame_off"][f]) + where[(f, p)]
    s["bridge_rows"] = [(row(fp, p), row(fq, q)) for p, fp, q, fq, _ in bridges]
    s["point_rows"] = {p: [row(f, p) for f in seen[p]] for p in seen}
    _scenes[key] = s
    return s


def chain_scene() -> dict:
    """Three points A, B, C seen in frames 0-3, 2-5 and 4-7; A's keypoint of frame 0 is bridged to B's of frame 4 and B's of
    frame 2 to C's of frame 6: one component of twelve rows."""
    return arc_scene("chain", {0: (0, 1, 2, 3), 1: (2, 3, 4, 5), 2: (4, 5, 6, 7)}, bridges=((0, 0, 1, 4, 1.5), (1, 2, 2, 6, 1.5)))


FAR = 2      # dead_scene's point whose two rays meet under less than 1.5 degrees


def dead_scene() -> dict:
    """Two glued points as in SR.glued_scene, and a point 80 away seen by the two middle frames only: its track of two entries is
    not accepted in round 0, so its rows are DEAD and no later round holds them."""
    return arc_scene("dead", {0: (0, 1, 2, 3), 1: (2, 3, 4, 5), FAR: (3, 4)}, bridges=((0, 0, 1, 4, 1.5),), fixed={FAR: (0.3, 0.2, 80.0)})


def lone_scene(n_lone: int) -> dict:
    """One point seen in frames 0-3 whose keypoint of frame 0 is bridged to ``n_lone`` keypoints of frame 4 that nothing else sees
    (at different depths along its ray): the leftover of round 0 is one row, or two rows of one frame with no edge between them."""
    seen = {0: (0, 1, 2, 3), **{1 + k: (4,) for k in range(n_lone)}}
    return arc_scene(f"lone{n_lone}", seen, bridges=tuple((0, 0, 1 + k, 4, 1.5 + 0.7 * k) for k in range(n_lone)))


SWEEP_SEED = 1
# name -> (scene, min_support, split_rounds): what tests/test_gpu_triangulation_split.py runs triangulate_map on, and
# tests/test_triangulation_split_cpu.py asserts the margins of
GPU_RUNS = {"glued": (SR.glued_scene, 0, 1), "chain": (chain_scene, 0, 3), "dead": (dead_scene, 0, 2), "lone1": (lambda: lone_scene(1), 0, 1),
            "lone2": (lambda: lone_scene(2), 0, 1), "sweep05": (lambda: SR.sweep_scene(0.05, SWEEP_SEED), 1, 2),
            "sweep10": (lambda: SR.sweep_scene(0.10, SWEEP_SEED), 1, 4)}


def gpu_run(name: str) -> tuple:
    fn, ms, R = GPU_RUNS[name]
    s = fn()
    return s, ms, R, run(s, ms, R)
