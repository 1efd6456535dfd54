"""Numpy restatement of the mapper's glue kernels (csrc/mapper.hip) in the kernels' order of operations, for the
tests of pram_amd.localization.mapper: the pair angles and their lower median (by sorting: the kernel's bisection must equal it),
the seed choice, the correspondences, the frame choice, the pack and the live edges.  Also the planted scene the CPU and GPU tests
share, built with the scene helpers of tests/triangulation_ref.py."""
from __future__ import annotations

import numpy as np

from tests import pose_ref as PR
from tests import triangulation_ref as TR

MAX_LINKS = 8      # PRAM_MAP_MAX_LINKS
DEFAULTS = dict(init_min_num_inliers=100, init_min_tri_angle=16.0, init_relax=2, min_corr=30, max_reg_trials=3, round_frames=0, max_corr=4096,
                abs_pose_max_error=12.0, abs_pose_min_num_inliers=30, abs_pose_min_inlier_ratio=0.25)
_IGN = dict(all="ignore")


# ---------------------------------------------------------------- stage 1
def match_angles(norm05, frame_off, f0: int, f1: int, kept, qvec, tvec, atan2=np.arctan2) -> np.ndarray:
    """Per kept match the triangulation angle (radians) under (qvec, tvec) of frame 1 from frame 0, nan where the match does not
    count: an index outside its frame, or a midpoint that is not in front of both cameras.  ``atan2``: the one elementary function
    of the chain that is not correctly rounded; the GPU test passes the device's, so that the angles are the kernel's to the bit."""
    kept = np.asarray(kept, dtype=np.int64).reshape(-1, 2)
    out = np.full(len(kept), np.nan)
    r0, r1 = int(frame_off[f0]), int(frame_off[f1])
    n0, n1 = int(frame_off[f0 + 1]) - r0, int(frame_off[f1 + 1]) - r1
    T = TR.frame_table(np.asarray(qvec, dtype=np.float64)[None], np.asarray(tvec, dtype=np.float64)[None], [0], [np.array([1.0, 0.0, 0.0])])[0]
    ok = (kept[:, 0] >= 0) & (kept[:, 0] < n0) & (kept[:, 1] >= 0) & (kept[:, 1] < n1)
    if not ok.any():
        return out
    with np.errstate(**_IGN):
        u0, v0 = norm05[r0 + kept[ok, 0]].T
        u1, v1 = norm05[r1 + kept[ok, 1]].T
        l0, l1 = np.sqrt(u0 * u0 + v0 * v0 + 1.0), np.sqrt(u1 * u1 + v1 * v1 + 1.0)
        d0 = [u0 / l0, v0 / l0, 1.0 / l0]
        x, y, z = u1 / l1, v1 / l1, 1.0 / l1
        d1 = [T[k] * x + T[3 + k] * y + T[6 + k] * z for k in range(3)]
        dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
        C0, C1 = [0.0, 0.0, 0.0], [T[12], T[13], T[14]]
        w = [C0[k] - C1[k] for k in range(3)]
        a, b, c, d, g = dot(d0, d0), dot(d0, d1), dot(d1, d1), dot(d0, w), dot(d1, w)
        den = a * c - b * b
        s, t = (b * g - c * d) / den, (a * g - b * d) / den
        X = [0.5 * ((C0[k] + s * d0[k]) + (C1[k] + t * d1[k])) for k in range(3)]
        z0, z1 = X[2], T[6] * X[0] + T[7] * X[1] + T[8] * X[2] + T[11]
        cr = [d0[1] * d1[2] - d0[2] * d1[1], d0[2] * d1[0] - d0[0] * d1[2], d0[0] * d1[1] - d0[1] * d1[0]]
        ang = np.asarray(atan2(np.sqrt(dot(cr, cr)), dot(d0, d1)), dtype=np.float64)
        out[ok] = np.where((z0 > 0.0) & (z1 > 0.0) & (ang >= 0.0), ang, np.nan)
    return out


def lower_median(angles) -> tuple:
    """(the number of angles that count, element (n - 1) // 2 of them in ascending order; 0.0 for none)."""
    a = np.sort(np.asarray(angles, dtype=np.float64)[~np.isnan(angles)])
    return len(a), (float(a[(len(a) - 1) // 2]) if len(a) else 0.0)


def bisect_median(angles) -> float:
    """The kernel's way to the same element: the largest 64-bit word with at most k words below it, bit by bit from the top."""
    a = np.asarray(angles, dtype=np.float64)
    words = a[~np.isnan(a)].view(np.uint64)
    if len(words) == 0:
        return 0.0
    k, med = (len(words) - 1) // 2, 0
    for bit in range(63, -1, -1):
        cand = med | (1 << bit)
        if int((words < np.uint64(cand)).sum()) <= k:
            med = cand
    return float(np.array([med], dtype=np.uint64).view(np.float64)[0])


def pair_angles(norm05, frame_off, pairs, kept, qvec, tvec, success, atan2=np.arctan2) -> tuple:
    """kept: per pair int [c, 2] -> (n_tri int32 [Pn], tri_angle float64 [Pn])."""
    n, ang = [], []
    for p, (f0, f1) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        ok = bool(success[p]) and 0 <= f0 < len(frame_off) - 1 and 0 <= f1 < len(frame_off) - 1
        c, m = lower_median(match_angles(norm05, frame_off, f0, f1, kept[p], qvec[p], tvec[p], atan2)) if ok else (0, 0.0)
        n.append(c); ang.append(m)
    return np.array(n, dtype=np.int32), np.array(ang, dtype=np.float64)


def seed(success, n_tri, tri_angle, min_num_inliers: int, min_tri_angle: float) -> int:
    """min_tri_angle in radians -> the eligible pair with the largest n_tri, the lowest position on a tie; -1: none."""
    best, at = -1, -1
    for p in range(len(n_tri)):
        if success[p] and n_tri[p] >= min_num_inliers and tri_angle[p] >= min_tri_angle and n_tri[p] > best:
            best, at = int(n_tri[p]), p
    return at


def seed_relaxed(success, n_tri, tri_angle, min_num_inliers: int, min_tri_angle_deg: float, relax: int) -> tuple:
    for k in range(relax + 1):
        s = seed(success, n_tri, tri_angle, min_num_inliers >> k, float(np.deg2rad(min_tri_angle_deg)) / 2 ** k)
        if s >= 0:
            return s, k
    return -1, relax


# ---------------------------------------------------------------- stage 3
def adjacency(n_rows: int, edges) -> tuple:
    """tri_adjacency's table: (adj_off [n_rows + 1], adj, every row's neighbours ascending, one entry per edge)."""
    lists = [[] for _ in range(n_rows)]
    for u, v in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        if 0 <= u < n_rows and 0 <= v < n_rows and u != v:
            lists[u].append(v); lists[v].append(u)
    off = np.zeros(n_rows + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.array([v for x in lists for v in sorted(x)], dtype=np.int32)


def _clamped(o0, o1, n: int) -> tuple:
    """glue.h's clamped_range: a CSR range cut into a table of n entries."""
    beg = min(max(int(o0), 0), n)
    return beg, max(beg, min(int(o1), n))


def correspond(adj_off, adj, row_frame, frame_off, registered, row_point, n_points: int) -> dict:
    F, n_rows = len(frame_off) - 1, len(row_frame)
    n_corr, dropped, rows, pts = np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32), [], []
    for f in range(F):
        if registered[f]:
            continue
        for u in range(*_clamped(frame_off[f], frame_off[f + 1], n_rows)):
            found = []
            for v in adj[slice(*_clamped(adj_off[u], adj_off[u + 1], len(adj)))].tolist():
                if not 0 <= v < n_rows:
                    continue
                fv = int(row_frame[v])
                if not 0 <= fv < F or not registered[fv]:
                    continue
                pt = int(row_point[v])
                if 0 <= pt < n_points:
                    found.append(pt)
            keep = sorted(set(found))[:MAX_LINKS]
            n_corr[f] += len(keep)
            dropped[f] += sum(1 for pt in found if pt > keep[-1]) if len(keep) == MAX_LINKS else 0
            rows += [u] * len(keep); pts += keep
    off = np.zeros(F + 1, dtype=np.int32)
    off[1:] = np.cumsum(n_corr)
    return {"n_corr": n_corr, "corr_off": off, "dropped": dropped, "corr_row": np.array(rows, dtype=np.int32), "corr_point": np.array(pts, dtype=np.int32)}


# ---------------------------------------------------------------- stage 4
def choose(n_corr, registered, tries, min_corr: int, max_reg_trials: int, round_frames: int) -> tuple:
    cand = [f for f in range(len(n_corr)) if not registered[f] and n_corr[f] >= max(min_corr, 1) and tries[f] < max_reg_trials]
    cand.sort(key=lambda f: (-int(n_corr[f]), f))
    if round_frames > 0:
        cand = cand[:round_frames]
    return np.array(cand, dtype=np.int32), np.array([n_corr[f] for f in cand], dtype=np.int32)


def pack(chosen, corr: dict, keypoints, xyz, t0: int) -> dict:
    S = len(chosen)
    kp, pts = np.zeros((S, t0, 2), dtype=np.float32), np.zeros((S, t0, 3), dtype=np.float64)
    counts, cut = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    for s, f in enumerate(np.asarray(chosen).tolist()):
        a, b = int(corr["corr_off"][f]), int(corr["corr_off"][f + 1])
        take = min(b - a, t0)
        counts[s], cut[s] = take, b - a - take
        kp[s, :take] = keypoints[corr["corr_row"][a:a + take]]
        pts[s, :take] = xyz[corr["corr_point"][a:a + take]]
    return {"matched_keypoints": kp, "matched_xyzs": pts, "counts": counts, "cut": cut}


# ---------------------------------------------------------------- stage 5
def live_edges(edges, row_frame, registered) -> np.ndarray:
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    n_rows, F = len(row_frame), len(registered)
    out = np.full(e.shape, -1, dtype=np.int32)
    for i, (u, v) in enumerate(e.tolist()):
        if 0 <= u < n_rows and 0 <= v < n_rows:
            fu, fv = int(row_frame[u]), int(row_frame[v])
            if 0 <= fu < F and 0 <= fv < F and registered[fu] and registered[fv]:
                out[i] = (u, v)
    return out


# ---------------------------------------------------------------- the planted scene
N_ARC, N_LINE = 12, 4
N_MAIN = N_ARC + N_LINE                      # frames 0 .. 15: the arc, then the straight line
F_ROT = N_MAIN                               # at frame 0's centre, rotated 10 degrees: its pair with frame 0 has the most matches
F_ISO = (N_MAIN + 1, N_MAIN + 2)             # matched only with each other: a second component
F_FEW = N_MAIN + 3                           # about ten of its matches lead into the map
N_FRAMES = N_MAIN + 4
F_HELD = (N_FRAMES, N_FRAMES + 1)            # two held-out views: in ``held``, not among the frames
N_POINTS, N_ISO_POINTS, N_FEW_PRIVATE, N_FEW_SHARED = 600, 20, 20, 10      # the frames left out see about 5 % of the points
WRONG_SHARE, NOISE_PX, MAX_GAP = 0.2, 0.5, 3
ARC_STEP_DEG, RADIUS, LINE_STEP = 7.0, 8.0, 1.0
_scene: dict = {}


def planted_scene(seed: int = 26) -> dict:
    """20 frames over the five camera models in turn: 12 on an arc and 4 that continue it in a straight line, matched with the
    frames at most three apart (20 % of a pair's matches are wrong, 0.5 px of noise); a frame at frame 0's centre rotated by 10
    degrees whose pair with frame 0 has the most matches of all; two frames matched only with each other; one frame of whose
    matches about ten lead into the map.  ``expected``: what the mapper must make of it."""
    if seed in _scene:
        return _scene[seed]
    rng = np.random.RandomState(seed)
    ang = np.deg2rad(-40.0 + ARC_STEP_DEG * np.arange(N_ARC))
    centres = [np.array([RADIUS * np.sin(a), 0.3 * np.cos(3 * a), -RADIUS * np.cos(a)]) for a in ang]
    tangent = np.array([np.cos(ang[-1]), 0.0, np.sin(ang[-1])])
    centres += [centres[N_ARC - 1] + LINE_STEP * (k + 1) * tangent for k in range(N_LINE)]
    targets = [np.zeros(3)] * N_MAIN
    c, s_ = np.cos(np.deg2rad(10.0)), np.sin(np.deg2rad(10.0))
    centres.append(centres[0].copy()); targets.append(centres[0] + np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]]) @ (np.zeros(3) - centres[0]))
    far = np.array([60.0, 0.0, 0.0])
    centres += [far + np.array([-1.5, 0.0, -8.0]), far + np.array([1.5, 0.1, -8.0])]; targets += [far, far]
    centres.append(np.array([0.6, -0.5, -8.6])); targets.append(np.zeros(3))
    held = [np.array([RADIUS * np.sin(a), -0.4, -0.95 * RADIUS * np.cos(a)]) for a in np.deg2rad([-21.0, 9.0])]
    F = N_FRAMES + len(held)
    s = TR._base([TR.CAMERAS[f % 5] for f in range(F)], centres + held, targets + [np.zeros(3)] * len(held))
    xyz = np.vstack([rng.uniform([-2.5, -1.5, -2.0], [2.5, 1.5, 2.0], size=(N_POINTS, 3)),
                     far + rng.uniform([-2.0, -1.4, -2.0], [2.0, 1.4, 2.0], size=(N_ISO_POINTS, 3)),
                     rng.uniform([-2.0, -1.4, -2.0], [2.0, 1.4, 2.0], size=(N_FEW_PRIVATE, 3))])
    main = np.arange(N_POINTS)
    iso = np.arange(N_POINTS, N_POINTS + N_ISO_POINTS)
    private = np.arange(N_POINTS + N_ISO_POINTS, len(xyz))
    vis = np.zeros((F, len(xyz)), dtype=bool)
    vis[:N_MAIN, :N_POINTS] = rng.uniform(size=(N_MAIN, N_POINTS)) < 0.8
    vis[0, :N_POINTS] = vis[F_ROT, :N_POINTS] = True
    vis[np.ix_(F_ISO, iso)] = True
    F_FEW_PARTNER = 5
    shared = rng.choice(np.nonzero(vis[F_FEW_PARTNER, :N_POINTS])[0], N_FEW_SHARED, replace=False)
    vis[F_FEW, shared] = True
    vis[np.ix_([F_FEW, F_FEW_PARTNER], private)] = True
    vis[N_FRAMES:, :N_POINTS] = True
    kps, where = [[] for _ in range(F)], {}
    for f in range(F):
        px, z = TR.project(s, f, xyz)
        for pt in rng.permutation(len(xyz)).tolist():
            if vis[f, pt] and z[pt] > 0.5 and 8.0 <= px[pt, 0] < TR.WIDTH - 8.0 and 8.0 <= px[pt, 1] < TR.HEIGHT - 8.0:
                kps[f].append(tuple(px[pt] - 0.5 + rng.normal(0.0, NOISE_PX, size=2)))
                where[(f, pt)] = len(kps[f]) - 1
            if f < N_FRAMES and rng.uniform() < 0.25:
                kps[f].append(tuple(rng.uniform([8.0, 8.0], [TR.WIDTH - 8.0, TR.HEIGHT - 8.0])))      # a detection of nothing
    pairs = [(a, b) for a in range(N_MAIN) for b in range(a + 1, min(a + MAX_GAP + 1, N_MAIN))] + [(0, F_ROT), F_ISO, (F_FEW_PARTNER, F_FEW)]
    matches, right = [], []
    for a, b in pairs:
        special = (a, b) in ((0, F_ROT), (F_FEW_PARTNER, F_FEW))
        share = 1.0 if special else 0.9
        good = [(where[(a, pt)], where[(b, pt)]) for pt in range(len(xyz)) if (a, pt) in where and (b, pt) in where and rng.uniform() < share]
        if (a, b) == (F_FEW_PARTNER, F_FEW):      # only the shared and the private points: about ten lead into the map
            good = [(where[(a, pt)], where[(b, pt)]) for pt in list(shared) + list(private) if (a, pt) in where and (b, pt) in where]
        m = list(good)
        if not special:      # wrong matches: a fifth of the pair's list, between keypoints no right match uses
            used0, used1 = {x[0] for x in m}, {x[1] for x in m}
            free0 = [i for i in rng.permutation(len(kps[a])).tolist() if i not in used0]
            free1 = [j for j in rng.permutation(len(kps[b])).tolist() if j not in used1]
            n_wrong = min(int(round(len(good) * WRONG_SHARE / (1.0 - WRONG_SHARE))), len(free0), len(free1))
            m += list(zip(free0[:n_wrong], free1[:n_wrong]))
        order = rng.permutation(len(m))
        matches.append([m[k] for k in order.tolist()])
        right.append(len(good))
    s.update(pairs=pairs, matches=matches, xyz=xyz, where=where, n_right=np.array(right), vis=vis, shared=shared, few_partner=F_FEW_PARTNER)
    s = TR._finish(s, kps)
    # the held-out views leave the frame list: their keypoints, cameras, poses and the planted point of every keypoint stay
    fo = s["frame_off"]
    s["held"] = [{"keypoints": s["keypoints"][fo[f]:fo[f + 1]], "camera": s["cameras"][f], "qvec": s["qvec"][f], "tvec": s["tvec"][f],
                  "points": np.array([pt for (g, pt), k in sorted(where.items(), key=lambda kv: kv[1]) if g == f])} for f in F_HELD]
    for k in ("cameras", "frames"):
        s[k] = s[k][:N_FRAMES]
    for k in ("cam_model", "cam_params", "qvec", "tvec", "table"):
        s[k] = s[k][:N_FRAMES]
    n = int(fo[N_FRAMES])
    s["keypoints"], s["norm0"], s["norm05"], s["frame_off"], s["n_frames"] = s["keypoints"][:n], s["norm0"][:n], s["norm05"][:n], fo[:N_FRAMES + 1], N_FRAMES
    s["expected"] = {"registered": np.array([f < N_MAIN or f == F_ROT for f in range(N_FRAMES)]),
                     "reasons": {F_ISO[0]: "no_correspondences", F_ISO[1]: "no_correspondences", F_FEW: "few_correspondences"},
                     "rotation_pair": pairs.index((0, F_ROT))}
    _scene[seed] = s
    return s


def true_relative(s: dict, f0: int, f1: int) -> tuple:
    """The planted (qvec, unit tvec) of frame f1 from frame f0."""
    R0, R1 = s["table"][f0, :9].reshape(3, 3), s["table"][f1, :9].reshape(3, 3)
    R = R1 @ R0.T
    t = s["table"][f1, 9:12] - R @ s["table"][f0, 9:12]
    n = np.linalg.norm(t)
    return PR.rot_to_qvec(R), (t / n if n > 0 else np.array([1.0, 0.0, 0.0]))


def centres_of(qvec, tvec) -> np.ndarray:
    return np.stack([-PR.qvec_to_rot(q).T @ t for q, t in zip(np.asarray(qvec), np.asarray(tvec))])


def pose_errors(res_q, res_t, s: dict, which, sRt) -> tuple:
    """The largest rotation error (degrees) and the largest centre error over the frames ``which`` after the similarity sRt."""
    sc, R, t = sRt
    rot, cen = 0.0, 0.0
    C = centres_of(res_q, res_t)
    for f in np.asarray(which).tolist():
        Rc = PR.qvec_to_rot(res_q[f]) @ R.T
        Rt = s["table"][f, :9].reshape(3, 3)
        cosv = np.clip((np.trace(Rc @ Rt.T) - 1.0) / 2.0, -1.0, 1.0)
        rot = max(rot, float(np.degrees(np.arccos(cosv))))
        cen = max(cen, float(np.linalg.norm(sc * R @ C[f] + t - s["table"][f, 12:15])))
    return rot, cen


def rotation_scene(seed: int = 27) -> dict:
    """Four frames at one centre, each turned 8 degrees further, matched all against all: every pair is a pure rotation and no
    pair may become a seed."""
    if ("rot", seed) in _scene:
        return _scene[("rot", seed)]
    rng = np.random.RandomState(seed)
    C = np.array([0.0, 0.0, -8.0])
    targets = [C + np.array([np.sin(a), 0.0, np.cos(a)]) for a in np.deg2rad([-12.0, -4.0, 4.0, 12.0])]
    s = TR._base([TR.CAMERAS[f % 5] for f in range(4)], [C] * 4, targets)
    xyz = rng.uniform([-2.5, -1.5, -2.0], [2.5, 1.5, 2.0], size=(300, 3))
    kps, where = [[] for _ in range(4)], {}
    for f in range(4):
        px, z = TR.project(s, f, xyz)
        for pt in rng.permutation(len(xyz)).tolist():
            if z[pt] > 0.5 and 8.0 <= px[pt, 0] < TR.WIDTH - 8.0 and 8.0 <= px[pt, 1] < TR.HEIGHT - 8.0:
                kps[f].append(tuple(px[pt] - 0.5 + rng.normal(0.0, NOISE_PX, size=2)))
                where[(f, pt)] = len(kps[f]) - 1
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    matches = [[(where[(a, pt)], where[(b, pt)]) for pt in range(len(xyz)) if (a, pt) in where and (b, pt) in where] for a, b in pairs]
    s.update(pairs=pairs, matches=matches, xyz=xyz)
    _scene[("rot", seed)] = TR._finish(s, kps)
    return _scene[("rot", seed)]


def planted_features(s: dict, noise: float = 0.25, seed: int = 28) -> tuple:
    """Descriptors for the planted scene, by the recipe of refine_ref.covisible_scene: a unit descriptor per planted point, every
    keypoint of that point the descriptor plus noise, a keypoint of nothing a descriptor of its own -> (the feature frames
    DatabaseStore.from_triangulation takes, the two held-out views as cand_ref's queries: the real rows, and ``padded`` to one length)."""
    rng = np.random.RandomState(seed)
    unit = lambda x: (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)
    desc = unit(rng.standard_normal((len(s["xyz"]), 128)))
    near = lambda pts: unit(desc[pts] + noise / np.sqrt(128.0) * rng.standard_normal((len(pts), 128)))
    fo, frames = s["frame_off"], []
    for f in range(s["n_frames"]):
        n = int(fo[f + 1] - fo[f])
        d = unit(rng.standard_normal((max(n, 1), 128)))[:n]
        own = [(k, pt) for (g, pt), k in s["where"].items() if g == f]
        if own:
            k, pt = np.array(own).T
            d[k] = near(pt)
        kp = np.concatenate([s["keypoints"][fo[f]:fo[f + 1]], rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1)
        frames.append({"keypoints": kp, "descriptors": d, "width": TR.WIDTH, "height": TR.HEIGHT})
    n_pad = max(len(h["keypoints"]) for h in s["held"])
    pad = lambda a: np.concatenate([a, np.zeros((n_pad - len(a),) + a.shape[1:], dtype=a.dtype)])
    queries = []
    for h in s["held"]:
        n = len(h["keypoints"])
        q = {"keypoints": h["keypoints"].astype(np.float32), "scores": rng.uniform(0, 1, n).astype(np.float32), "descriptors": near(h["points"]),
             "count": n, "width": TR.WIDTH, "height": TR.HEIGHT}
        q["padded"] = {k: pad(q[k]) for k in ("keypoints", "scores", "descriptors")}
        queries.append(q)
    return frames, queries
