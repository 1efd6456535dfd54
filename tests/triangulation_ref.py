"""Numpy float64 restatement of the triangulation stages (csrc/triangulate.hip), for the tests of
pram_amd.localization.triangulation: normalised keypoints, the epipolar test, connected components, the track table and the robust
solve of one track, which also returns a trace of the branches it took.  Plain host code written from the formulas; sums that the
kernel runs per lane and combines by a butterfly are run the same way here (:func:`wave_sum`), so the two differ by the rounding
of the compiler's and numpy's elementary operations only.  Also the seeded scenes the CPU and GPU tests share."""
from __future__ import annotations

import numpy as np

from tests import pose_ref as PR

GN_STEPS = 5          # PRAM_TRI_GN_STEPS
FRAME_COLS = 16       # PRAM_TRI_FRAME_COLS
DEFAULTS = dict(max_error=4.0, trials=128, seed=0, min_tri_angle=1.5, max_reproj_error=4.0)
_IGN = dict(all="ignore")


# ---------------------------------------------------------------- stage 1: the frame table and the normalised keypoints
def frame_table(qvec, tvec, cam_model, cam_params) -> np.ndarray:
    q = np.asarray(qvec, dtype=np.float64)
    t = np.asarray(tvec, dtype=np.float64)
    nq = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    w, x, y, z = (q[:, k] / nq for k in range(4))
    T = np.zeros((q.shape[0], FRAME_COLS))
    T[:, 0] = 1.0 - 2.0 * y * y - 2.0 * z * z; T[:, 1] = 2.0 * x * y - 2.0 * w * z; T[:, 2] = 2.0 * z * x + 2.0 * w * y
    T[:, 3] = 2.0 * x * y + 2.0 * w * z; T[:, 4] = 1.0 - 2.0 * x * x - 2.0 * z * z; T[:, 5] = 2.0 * y * z - 2.0 * w * x
    T[:, 6] = 2.0 * z * x - 2.0 * w * y; T[:, 7] = 2.0 * y * z + 2.0 * w * x; T[:, 8] = 1.0 - 2.0 * x * x - 2.0 * y * y
    T[:, 9:12] = t
    for k in range(3):
        T[:, 12 + k] = -(T[:, k] * t[:, 0] + T[:, 3 + k] * t[:, 1] + T[:, 6 + k] * t[:, 2])
    T[:, 15] = [PR.f_mean(int(m), p) for m, p in zip(cam_model, cam_params)]
    return T


def normalize(kpts, frame_off, cam_model, cam_params, off: float) -> np.ndarray:
    """float32 keypoints [n_rows, 2] -> [n_rows, 2] on each row's normalised plane, (x + off, y + off) undistorted."""
    k = np.asarray(kpts, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    out = np.zeros_like(k)
    for f in range(len(frame_off) - 1):
        a, b = int(frame_off[f]), int(frame_off[f + 1])
        fx, fy, cx, cy, k1, k2, p1, p2 = PR.unify(int(cam_model[f]), cam_params[f])
        u, v = PR.undistort(((k[a:b, 0] + off) - cx) / fx, ((k[a:b, 1] + off) - cy) / fy, k1, k2, p1, p2)
        out[a:b, 0], out[a:b, 1] = u, v
    return out


# ---------------------------------------------------------------- stage 2: the epipolar test
def essential(T0, T1) -> np.ndarray:
    """E = [t / |t|]x R of cam1_from_cam0, from two rows of the frame table."""
    A, B = T0, T1
    R = np.array([[B[a * 3] * A[c * 3] + B[a * 3 + 1] * A[c * 3 + 1] + B[a * 3 + 2] * A[c * 3 + 2] for c in range(3)] for a in range(3)])
    t = np.array([B[9 + a] - (R[a, 0] * A[9] + R[a, 1] * A[10] + R[a, 2] * A[11]) for a in range(3)])
    with np.errstate(**_IGN):
        x, y, z = t / np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    return np.array([y * R[2] - z * R[1], z * R[0] - x * R[2], x * R[1] - y * R[0]])


def epipolar_errors(E, x0, x1):
    """compute_epipolar_errors of colmap_utils/geometry.py, written out: x0 / x1 [m, 2] normalised points of frame 0 / 1."""
    u0, v0, u1, v1 = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    lj0, lj1 = E[0, 0] * u0 + E[0, 1] * v0 + E[0, 2], E[1, 0] * u0 + E[1, 1] * v0 + E[1, 2]
    li0, li1, li2 = E[0, 0] * u1 + E[1, 0] * v1 + E[2, 0], E[0, 1] * u1 + E[1, 1] * v1 + E[2, 1], E[0, 2] * u1 + E[1, 2] * v1 + E[2, 2]
    dist = np.abs(u0 * li0 + v0 * li1 + li2)
    with np.errstate(**_IGN):
        return dist / np.sqrt(li0 * li0 + li1 * li1), dist / np.sqrt(lj0 * lj0 + lj1 * lj1)


def unique_pairs(pairs) -> list:
    seen, keep = set(), []
    for i, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        if (a, b) in seen or (b, a) in seen:
            continue
        seen |= {(a, b), (b, a)}
        keep.append(i)
    return keep


def verify(norm0, frame_off, table, pairs, matches, max_error: float = 4.0) -> dict:
    """pairs [Pn, 2] (already unique), matches: per pair int [m, 2] -> per pair keep / kept / errors / thresholds / in-range mask,
    and the edges (rows) of all kept matches in pair order."""
    out = {"keep": [], "kept": [], "count": [], "errors": [], "thresholds": [], "in_range": [], "edges": []}
    for (f0, f1), m in zip(np.asarray(pairs).reshape(-1, 2).tolist(), matches):
        m = np.asarray(m, dtype=np.int64).reshape(-1, 2)
        r0, r1 = int(frame_off[f0]), int(frame_off[f1])
        n0, n1 = int(frame_off[f0 + 1]) - r0, int(frame_off[f1 + 1]) - r1
        ok = (m[:, 0] >= 0) & (m[:, 0] < n0) & (m[:, 1] >= 0) & (m[:, 1] < n1)
        e0, e1 = np.full(len(m), np.inf), np.full(len(m), np.inf)
        if ok.any():
            e0[ok], e1[ok] = epipolar_errors(essential(table[f0], table[f1]), norm0[r0 + m[ok, 0]], norm0[r1 + m[ok, 1]])
        th = (max_error / table[f0, 15], max_error / table[f1, 15])
        keep = ok & (e0 <= th[0]) & (e1 <= th[1])
        out["keep"].append(keep); out["kept"].append(m[keep]); out["count"].append(int(keep.sum()))
        out["errors"].append(np.stack([e0, e1], 1)); out["thresholds"].append(th); out["in_range"].append(ok)
        out["edges"].append(np.stack([r0 + m[keep, 0], r1 + m[keep, 1]], 1))
    out["edges"] = np.concatenate(out["edges"]) if out["edges"] else np.zeros((0, 2), dtype=np.int64)
    return out


# ---------------------------------------------------------------- stage 3: components and tracks
def components(n_rows: int, edges) -> np.ndarray:
    """label [n_rows]: the smallest row of every row's component."""
    parent = list(range(n_rows))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        if u < 0 or v < 0 or u >= n_rows or v >= n_rows:
            continue
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n_rows)], dtype=np.int32)


def tracks(label, frame_off) -> dict:
    label = np.asarray(label, dtype=np.int64)
    size = np.bincount(label, minlength=len(label)) if len(label) else np.zeros(0, dtype=np.int64)
    labs = np.nonzero(size >= 2)[0]
    rows = [np.nonzero(label == l)[0] for l in labs.tolist()]
    off = np.zeros(len(labs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    row = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)
    frame = (np.searchsorted(np.asarray(frame_off), row, side="right") - 1).astype(np.int32)
    return {"trk_off": off, "trk_label": labs.astype(np.int32), "trk_row": row, "trk_frame": frame,
            "trk_kpt": (row - np.asarray(frame_off)[frame]).astype(np.int32)}


# ---------------------------------------------------------------- stage 4: one track
def wave_sum(v):
    """Sum over the leading axis as a wave does: lane l adds entries l, l + 64, ... in ascending order, then the xor butterfly."""
    v = np.asarray(v, dtype=np.float64)
    part = np.zeros((64,) + v.shape[1:])
    for k in range(v.shape[0]):
        part[k % 64] = part[k % 64] + v[k]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[lanes ^ o]
    return part[0]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def angle(a, b) -> float:
    c = _cross(a, b)
    return float(np.arctan2(np.sqrt(_dot(c, c)), _dot(a, b)))


def chol_solve3(A, b):
    """A: a00 a01 a02 a11 a12 a22 -> x or None."""
    with np.errstate(**_IGN):
        if not A[0] > 0.0:
            return None
        l00 = np.sqrt(A[0]); l10 = A[1] / l00; l20 = A[2] / l00
        d1 = A[3] - l10 * l10
        if not d1 > 0.0:
            return None
        l11 = np.sqrt(d1); l21 = (A[4] - l20 * l10) / l11
        d2 = A[5] - l20 * l20 - l21 * l21
        if not d2 > 0.0:
            return None
        l22 = np.sqrt(d2)
        y0 = b[0] / l00; y1 = (b[1] - l10 * y0) / l11; y2 = (b[2] - l20 * y0 - l21 * y1) / l22
        x2 = y2 / l22; x1 = (y1 - l21 * x2) / l11; x0 = (y0 - l10 * x1 - l20 * x2) / l00
    x = np.array([x0, x1, x2])
    return x if np.isfinite(x).all() else None


class Track:
    """The entries of one track with everything the solve reads of them."""

    def __init__(self, scene: dict, rows, frames):
        self.rows, self.frames = np.asarray(rows, dtype=np.int64), np.asarray(frames, dtype=np.int64)
        self.T = scene["table"][self.frames]
        self.cam = np.array([PR.unify(int(scene["cam_model"][f]), scene["cam_params"][f]) for f in self.frames]).reshape(-1, 8)
        self.obs = scene["keypoints"][self.rows].astype(np.float64) + 0.5
        uv = scene["norm05"][self.rows]
        n = np.sqrt(uv[:, 0] * uv[:, 0] + uv[:, 1] * uv[:, 1] + 1.0)
        x, y, z = uv[:, 0] / n, uv[:, 1] / n, 1.0 / n
        T = self.T
        self.ray = np.stack([T[:, k] * x + T[:, 3 + k] * y + T[:, 6 + k] * z for k in range(3)], 1)
        self.C = T[:, 12:15]

    def depth(self, X):
        T = self.T
        return T[:, 6] * X[0] + T[:, 7] * X[1] + T[:, 8] * X[2] + T[:, 11]

    def residual(self, X, with_jac: bool = False):
        T, c = self.T, self.cam
        with np.errstate(**_IGN):
            xc = T[:, 0] * X[0] + T[:, 1] * X[1] + T[:, 2] * X[2] + T[:, 9]
            yc = T[:, 3] * X[0] + T[:, 4] * X[1] + T[:, 5] * X[2] + T[:, 10]
            z = self.depth(X)
            u, v = xc / z, yc / z
            ud, vd = PR.distort(u, v, c[:, 4], c[:, 5], c[:, 6], c[:, 7])
            r0, r1 = c[:, 0] * ud + c[:, 2] - self.obs[:, 0], c[:, 1] * vd + c[:, 3] - self.obs[:, 1]
            if not with_jac:
                return z, r0, r1
            j11, j12, _, j22 = PR.distort_jac(u, v, c[:, 4], c[:, 5], c[:, 6], c[:, 7])
            iz = 1.0 / z
            a00, a01, a02 = c[:, 0] * j11 * iz, c[:, 0] * j12 * iz, -c[:, 0] * (j11 * u + j12 * v) * iz
            a10, a11, a12 = c[:, 1] * j12 * iz, c[:, 1] * j22 * iz, -c[:, 1] * (j12 * u + j22 * v) * iz
            J = np.stack([a00 * T[:, k] + a01 * T[:, 3 + k] + a02 * T[:, 6 + k] for k in range(3)]
                         + [a10 * T[:, k] + a11 * T[:, 3 + k] + a12 * T[:, 6 + k] for k in range(3)], 1)
        return z, r0, r1, J

    def inliers(self, X, thr2: float):
        z, r0, r1 = self.residual(X)
        with np.errstate(**_IGN):
            e2 = r0 * r0 + r1 * r1
            return (z > 0.0) & (e2 <= thr2), e2


def hypothesis_pairs(L: int, label: int, trials: int, seed: int):
    """(exhaustive, [(i, j)] with i < j): every pair in lexicographic order within the budget, else the sampler's draws."""
    if L * (L - 1) // 2 <= trials:
        return True, [(i, j) for i in range(L) for j in range(i + 1, L)]
    tr = np.arange(trials)
    a = PR.mulhi(PR.draw_u64(seed, label, tr, 0), L)
    b = PR.mulhi(PR.draw_u64(seed, label, tr, 1), L - 1)
    b = b + (b >= a)
    return False, list(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))


def triangulate_track(scene: dict, rows, frames, label: int, trials: int = 128, seed: int = 0, min_tri_angle: float = 1.5,
                      max_reproj_error: float = 4.0) -> dict:
    """-> accept, xyz, error, kept, best, entry_keep, entry_error and ``trace``: the branches taken and every quantity that was
    compared with a threshold (``angles`` in radians, ``reproj`` in pixels, ``hyps`` = (index, i, j, inliers, sse))."""
    tk = Track(scene, rows, frames)
    L = len(tk.rows)
    min_angle, thr2 = float(np.deg2rad(min_tri_angle)), max_reproj_error * max_reproj_error
    exhaustive, prs = hypothesis_pairs(L, label, trials, seed) if L >= 2 else (True, [])
    tr = {"L": L, "exhaustive": exhaustive, "same_frame": 0, "low_angle": 0, "bad_depth": 0, "few_inliers": 0, "hyps": [], "angles": [],
          "reproj": [], "ls_ok": None, "gn_taken": [], "deduped": 0, "accept_angle": None}
    best = (0, 0.0, -1, None)
    for h, (i, j) in enumerate(prs):
        if tk.frames[i] == tk.frames[j]:
            tr["same_frame"] += 1
            continue
        C1, C2, d1, d2 = tk.C[i], tk.C[j], tk.ray[i], tk.ray[j]
        ang = angle(d1, d2)
        tr["angles"].append(ang)
        if not ang >= min_angle:
            tr["low_angle"] += 1
            continue
        w = C1 - C2
        a, b, c, d, e = _dot(d1, d1), _dot(d1, d2), _dot(d2, d2), _dot(d1, w), _dot(d2, w)
        den = a * c - b * b
        s, u = (b * e - c * d) / den, (a * e - b * d) / den
        X = 0.5 * ((C1 + s * d1) + (C2 + u * d2))
        dz = tk.depth(X)
        if not dz[i] > 0.0 or not dz[j] > 0.0:
            tr["bad_depth"] += 1
            continue
        inl, e2 = tk.inliers(X, thr2)
        tr["reproj"].extend(np.sqrt(e2[np.isfinite(e2)]).tolist())
        cnt, sse = int(inl.sum()), float(wave_sum(np.where(inl, e2, 0.0)))
        tr["hyps"].append((h, i, j, cnt, sse))
        if cnt < 2:
            tr["few_inliers"] += 1
            continue
        if cnt > best[0] or (cnt == best[0] and sse < best[1]):
            best = (cnt, sse, h, X)
    out = {"accept": False, "xyz": np.zeros(3), "error": 0.0, "kept": 0, "best": best[2], "entry_keep": np.zeros(L, dtype=bool),
           "entry_error": np.full(L, -1.0), "trace": tr}
    if best[2] < 0:
        return out
    bX = best[3]
    inl, _ = tk.inliers(bX, thr2)
    dd, C = tk.ray, tk.C
    m00, m01, m02 = 1.0 - dd[:, 0] * dd[:, 0], -dd[:, 0] * dd[:, 1], -dd[:, 0] * dd[:, 2]
    m11, m12, m22 = 1.0 - dd[:, 1] * dd[:, 1], -dd[:, 1] * dd[:, 2], 1.0 - dd[:, 2] * dd[:, 2]
    terms = np.stack([m00, m01, m02, m11, m12, m22, m00 * C[:, 0] + m01 * C[:, 1] + m02 * C[:, 2],
                      m01 * C[:, 0] + m11 * C[:, 1] + m12 * C[:, 2], m02 * C[:, 0] + m12 * C[:, 1] + m22 * C[:, 2]], 1)
    acc = wave_sum(np.where(inl[:, None], terms, 0.0))
    x = chol_solve3(acc[:6], acc[6:])
    tr["ls_ok"] = x is not None
    X = x if x is not None else bX
    for _ in range(GN_STEPS):
        z, r0, r1, J = tk.residual(X, with_jac=True)
        with np.errstate(**_IGN):
            use = inl & (z > 1e-12) & np.isfinite(r0 * r0 + r1 * r1)
            terms = np.stack([J[:, 0] * J[:, 0] + J[:, 3] * J[:, 3], J[:, 0] * J[:, 1] + J[:, 3] * J[:, 4], J[:, 0] * J[:, 2] + J[:, 3] * J[:, 5],
                              J[:, 1] * J[:, 1] + J[:, 4] * J[:, 4], J[:, 1] * J[:, 2] + J[:, 4] * J[:, 5], J[:, 2] * J[:, 2] + J[:, 5] * J[:, 5],
                              -(J[:, 0] * r0 + J[:, 3] * r1), -(J[:, 1] * r0 + J[:, 4] * r1), -(J[:, 2] * r0 + J[:, 5] * r1)], 1)
        acc = wave_sum(np.where(use[:, None], terms, 0.0))
        x = chol_solve3(acc[:6], acc[6:])
        tr["gn_taken"].append(x is not None)
        if x is not None:
            X = X + x
    inl, e2 = tk.inliers(X, thr2)
    tr["reproj"].extend(np.sqrt(e2[np.isfinite(e2)]).tolist())
    err = np.where(inl, np.sqrt(np.where(inl, e2, 0.0)), -1.0)
    keep = inl.copy()
    for k in np.nonzero(inl)[0].tolist():      # one entry per frame: the smallest error, the lowest row on a tie
        same = np.nonzero(inl & (tk.frames == tk.frames[k]))[0]
        if any((err[o] < err[k]) or (err[o] == err[k] and o < k) for o in same.tolist() if o != k):
            keep[k] = False
    tr["deduped"] = int(inl.sum() - keep.sum())
    cnt = int(keep.sum())
    kept = np.nonzero(keep)[0].tolist()
    pair_angles = [angle(X - tk.C[a], X - tk.C[b]) for n_, a in enumerate(kept) for b in kept[n_ + 1:]]
    tr["angles"].extend(pair_angles)
    tr["accept_angle"] = any(a >= min_angle for a in pair_angles)
    out.update(accept=cnt >= 2 and tr["accept_angle"], xyz=X, kept=cnt, entry_keep=keep, entry_error=err,
               error=float(wave_sum(np.where(keep, err, 0.0))) / cnt if cnt else 0.0)
    return out


def triangulate(scene: dict, trk: dict, **params) -> dict:
    """Every track of ``trk`` -> the arrays pram_tri_triangulate writes, and ``traces``."""
    T = len(trk["trk_off"]) - 1
    res = [triangulate_track(scene, trk["trk_row"][a:b], trk["trk_frame"][a:b], int(l), **params)
           for a, b, l in zip(trk["trk_off"][:-1], trk["trk_off"][1:], trk["trk_label"])]
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.zeros(0, dtype=dt)
    return {"accept": np.array([r["accept"] for r in res], dtype=bool).reshape(T), "xyz": np.array([r["xyz"] for r in res]).reshape(T, 3),
            "error": np.array([r["error"] for r in res]).reshape(T), "kept": np.array([r["kept"] for r in res], dtype=np.int32).reshape(T),
            "best": np.array([r["best"] for r in res], dtype=np.int32).reshape(T), "entry_keep": cat("entry_keep", bool),
            "entry_error": cat("entry_error", np.float64), "traces": [r["trace"] for r in res]}


def run(scene: dict, **params) -> dict:
    """Stages 2-4 on a scene (stage 1 is in the scene) -> verify / label / tracks / tri."""
    p = {**DEFAULTS, **params}
    use = unique_pairs(scene["pairs"])
    v = verify(scene["norm0"], scene["frame_off"], scene["table"], scene["pairs"][use], [scene["matches"][i] for i in use], p["max_error"])
    label = components(int(scene["frame_off"][-1]), v["edges"])
    trk = tracks(label, scene["frame_off"])
    tri = triangulate(scene, trk, trials=p["trials"], seed=p["seed"], min_tri_angle=p["min_tri_angle"], max_reproj_error=p["max_reproj_error"])
    return {"pair_index": use, "verify": v, "label": label, "tracks": trk, "tri": tri}


# ---------------------------------------------------------------- scenes
WIDTH, HEIGHT = 640, 480
CAMERAS = (("SIMPLE_PINHOLE", WIDTH, HEIGHT, [515.0, 320.5, 239.0]), ("PINHOLE", WIDTH, HEIGHT, [520.0, 512.0, 318.0, 242.5]),
           ("SIMPLE_RADIAL", WIDTH, HEIGHT, [508.0, 321.0, 238.0, -0.05]), ("RADIAL", WIDTH, HEIGHT, [525.0, 319.0, 241.0, -0.06, 0.02]),
           ("OPENCV", WIDTH, HEIGHT, [518.0, 522.0, 322.0, 237.0, -0.05, 0.015, 0.001, -0.0008]))


def look_at(centre, target, up=(0.0, -1.0, 0.0)):
    """cam_from_world (R, t) of a camera at ``centre`` whose z axis points at ``target`` (x right, y down)."""
    centre, target = np.asarray(centre, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(-np.asarray(up), z)      # y down: x = down x forward ... right-handed with y = z x x
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ centre


def project(scene: dict, f: int, X):
    """World points [n, 3] -> (pixels in COLMAP's frame [n, 2], depths) through the full model of frame f."""
    R = scene["table"][f, :9].reshape(3, 3)
    return PR.project(np.asarray(X, dtype=np.float64).reshape(-1, 3), R, scene["table"][f, 9:12], int(scene["cam_model"][f]), scene["cam_params"][f])


def _base(cameras, centres, targets) -> dict:
    F = len(cameras)
    rows = [PR.camera_row(c) for c in cameras]
    s = {"cameras": list(cameras), "cam_model": np.array([r[0] for r in rows], dtype=np.int32), "cam_params": np.stack([r[1] for r in rows])}
    Rt = [look_at(c, t) for c, t in zip(centres, targets)]
    s["qvec"] = np.stack([PR.rot_to_qvec(R) for R, _ in Rt])
    s["tvec"] = np.stack([t for _, t in Rt])
    s["table"] = frame_table(s["qvec"], s["tvec"], s["cam_model"], s["cam_params"])
    s["n_frames"] = F
    return s


def _finish(s: dict, kps: list) -> dict:
    """kps: per frame a list of (x, y) stored keypoints -> keypoints, frame_off, frames and both normalisations."""
    lens = [len(k) for k in kps]
    s["frame_off"] = np.zeros(len(kps) + 1, dtype=np.int32)
    s["frame_off"][1:] = np.cumsum(lens)
    s["keypoints"] = np.array([p for k in kps for p in k], dtype=np.float32).reshape(-1, 2)
    s["frames"] = [{"keypoints": s["keypoints"][a:b]} for a, b in zip(s["frame_off"][:-1], s["frame_off"][1:])]
    s["norm0"] = normalize(s["keypoints"], s["frame_off"], s["cam_model"], s["cam_params"], 0.0)
    s["norm05"] = normalize(s["keypoints"], s["frame_off"], s["cam_model"], s["cam_params"], 0.5)
    s["pairs"] = np.asarray(s["pairs"], dtype=np.int64).reshape(-1, 2)
    s["matches"] = [np.asarray(m, dtype=np.int64).reshape(-1, 2) for m in s["matches"]]
    return s


N_ARC, F_OPPOSITE, F_EMPTY = 10, 10, 11      # frames 0..9 on an arc, frame 10 faces them, frame 11 has no keypoint
NOISE = 0.4                                  # keypoint noise: uniform in [-NOISE, NOISE] pixels per coordinate
_scenes: dict = {}


def tri_scene(noise: float = NOISE, seed: int = 11) -> dict:
    """12 frames over the five camera models, about 300 planted points and the special cases the tests name (``special``)."""
    key = ("tri", noise, seed)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.RandomState(seed)
    ang = np.deg2rad(np.linspace(-45.0, 45.0, N_ARC))
    centres = [np.array([8.0 * np.sin(a), 0.3 * np.cos(3 * a), -8.0 * np.cos(a)]) for a in ang] + [np.array([0.5, -0.2, 8.5]), np.array([0.0, 0.0, -9.0])]
    F = len(centres)
    s = _base([CAMERAS[f % 5] for f in range(F)], centres, [np.zeros(3)] * F)
    n_pts = 300
    xyz = rng.uniform([-2.0, -1.4, -2.0], [2.0, 1.4, 2.0], size=(n_pts, 3))
    far = n_pts                                  # a point whose rays all meet far below 1.5 degrees
    xyz = np.vstack([xyz, [[3.0, 1.0, 420.0]]])
    kps = [[] for _ in range(F)]
    where = {}                                   # (frame, point) -> keypoint index

    def add(f, xy, pid=None):
        kps[f].append((float(xy[0]), float(xy[1])))
        if pid is not None:
            where[(f, pid)] = len(kps[f]) - 1
        return len(kps[f]) - 1

    chain, dup, online = 0, 1, 2                 # planted points with a special role
    vis = rng.uniform(size=(F, len(xyz))) < 0.55
    vis[:, chain] = False; vis[0:5, chain] = True
    vis[:, dup] = False; vis[[1, 2, 3], dup] = True
    vis[:, online] = False; vis[[4, 5, 6], online] = True
    vis[:, far] = False; vis[[3, 4, 5], far] = True
    vis[F_EMPTY, :] = False
    for f in range(F):
        if f == F_EMPTY:
            continue
        px, z = project(s, f, xyz)
        order = rng.permutation(len(xyz))
        for p in order.tolist():
            inside = z[p] > 0.5 and 8.0 <= px[p, 0] < WIDTH - 8.0 and 8.0 <= px[p, 1] < HEIGHT - 8.0
            if vis[f, p] and inside:
                add(f, px[p] - 0.5 + rng.uniform(-noise, noise, size=2), p)      # stored keypoints: COLMAP's pixel minus 0.5
            if rng.uniform() < 0.15:
                add(f, rng.uniform([8.0, 8.0], [WIDTH - 8.0, HEIGHT - 8.0]))        # a detection of nothing
    special = {"chain": chain, "dup": dup, "online": online, "far": far}

    # a second detection of `dup` in frame 2, 0.9 px away, matched from frame 3 only
    px, _ = project(s, 2, xyz[dup])
    dup_kpt = add(2, px[0] - 0.5 + np.array([0.9, 0.0]))
    # a wrong match ON the epipolar line: a keypoint of frame 7 where another depth along `online`'s ray of frame 4 projects
    T4 = s["table"][4]
    k4 = np.array(kps[4][where[(4, online)]], dtype=np.float32).astype(np.float64)
    n4 = normalize(k4[None], [0, 1], s["cam_model"][4:5], s["cam_params"][4:5], 0.0)[0]
    ray4 = T4[:9].reshape(3, 3).T @ np.array([n4[0], n4[1], 1.0])
    depth4 = float(project(s, 4, xyz[online])[1][0])
    px, z = project(s, 7, T4[12:15] + 1.35 * depth4 * ray4)
    assert z[0] > 0 and 0 <= px[0, 0] < WIDTH and 0 <= px[0, 1] < HEIGHT
    online_kpt = add(7, px[0])
    # a point behind camera 4: frames 4 and 10 face each other; the rays meet behind camera 4
    k_behind4 = add(4, (331.0, 236.0))
    n4 = normalize(np.array([[331.0, 236.0]], dtype=np.float32), [0, 1], s["cam_model"][4:5], s["cam_params"][4:5], 0.0)[0]
    ray4 = T4[:9].reshape(3, 3).T @ np.array([n4[0], n4[1], 1.0])
    px, z = project(s, F_OPPOSITE, T4[12:15] - 2.0 * ray4)
    assert z[0] > 0 and 0 <= px[0, 0] < WIDTH and 0 <= px[0, 1] < HEIGHT
    k_behind10 = add(F_OPPOSITE, px[0])

    # ---- the pair list: neighbours on the arc, the facing frame against a few, one pair twice in both orders, one empty pair
    pairs = [(a, b) for a in range(N_ARC) for b in range(a + 1, min(a + 4, N_ARC))] + [(F_OPPOSITE, 2), (4, F_OPPOSITE), (F_OPPOSITE, 7)]
    pairs += [(3, 1), (0, F_EMPTY)]      # (1, 3) again in the other order; a frame without keypoints
    s_tmp = _finish(dict(s, pairs=pairs, matches=[[] for _ in pairs]), kps)
    matches = []
    wrong = 0
    for a, b in pairs:
        m = []
        for p in range(len(xyz)):
            if (a, p) in where and (b, p) in where and rng.uniform() < 0.85:
                m.append((where[(a, p)], where[(b, p)]))
        if abs(a - b) != 1:                         # `chain` is matched between neighbouring frames only: 0-1, 1-2, 2-3, 3-4
            m = [x for x in m if x != (where.get((a, chain)), where.get((b, chain)))]
        if (a, b) in ((1, 2), (1, 3), (2, 3)):      # `dup` is matched 1-2 and 1-3, its second detection in frame 2 from frame 3 only
            m = [x for x in m if x[0] != where.get((a, dup))]
            if (a, b) in ((1, 2), (1, 3)):
                m.append((where[(a, dup)], where[(b, dup)]))
            else:
                m.append((dup_kpt, where[(3, dup)]))
        if abs(a - b) == 1 and a < 5 and b < 5 and (where[(a, chain)], where[(b, chain)]) not in m:
            m.append((where[(a, chain)], where[(b, chain)]))
        if (a, b) == (4, 7):
            m = [x for x in m if x[0] != where[(4, online)]] + [(where[(4, online)], online_kpt)]
        if (a, b) in ((4, 5), (4, 6), (5, 6)) and (where[(a, online)], where[(b, online)]) not in m:
            m.append((where[(a, online)], where[(b, online)]))
        if (a, b) in ((3, 4), (4, 5), (3, 5)) and (where[(a, far)], where[(b, far)]) not in m:
            m.append((where[(a, far)], where[(b, far)]))
        if (a, b) == (4, F_OPPOSITE):
            m.append((k_behind4, k_behind10))
        # wrong matches that fail the epipolar test, chosen among detections of nothing and far from the line
        if a < N_ARC and b < N_ARC and len(kps[a]) and len(kps[b]):
            E = essential(s["table"][a], s["table"][b])
            th = 4.0 / min(s["table"][a, 15], s["table"][b, 15])
            used0, used1 = {x[0] for x in m}, {x[1] for x in m}
            for _ in range(6):
                i, j = int(rng.randint(len(kps[a]))), int(rng.randint(len(kps[b])))
                r0, r1 = s_tmp["frame_off"][a] + i, s_tmp["frame_off"][b] + j
                if i in used0 or j in used1:
                    continue
                e0, e1 = epipolar_errors(E, s_tmp["norm0"][r0:r0 + 1], s_tmp["norm0"][r1:r1 + 1])
                if min(e0[0], e1[0]) > 5.0 * th:
                    m.append((i, j)); used0.add(i); used1.add(j); wrong += 1
        if (a, b) == (0, 1):
            m += [(-1, 3), (2, len(kps[1])), (len(kps[0]), 0)]      # indices of -1 and of n
        order = rng.permutation(len(m))
        matches.append([m[k] for k in order.tolist()])
    s.update(pairs=pairs, matches=matches, xyz=xyz, where=where, special=special, n_wrong=wrong, noise=noise,
             special_rows={"dup_kpt": (2, dup_kpt), "online_kpt": (7, online_kpt), "behind": ((4, k_behind4), (F_OPPOSITE, k_behind10))})
    _scenes[key] = _finish(s, kps)
    return _scenes[key]


REVERSED_PAIR = (2, 4)      # stored as 4/2 in match_store


def frame_name(f: int) -> str:
    return f"seq/frame_{f:02d}.jpg"


def match_store(s: dict):
    """The scene's processed pairs as the matcher writes them: ``matches0`` per pair in a formats.DictStore, names from
    :func:`frame_name`; REVERSED_PAIR is stored under the other order.  Matches that ``matches0`` cannot hold (an index outside
    its frame) are left out -> (store, [(pair position, the matches stored, as a set of rows)])."""
    from pram_amd.localization import formats
    store, held = formats.DictStore(), []
    for i in unique_pairs(s["pairs"]):
        a, b = s["pairs"][i].tolist()
        n = [int(s["frame_off"][f + 1] - s["frame_off"][f]) for f in (a, b)]
        m = s["matches"][i]
        m = m[(m[:, 0] >= 0) & (m[:, 0] < n[0]) & (m[:, 1] >= 0) & (m[:, 1] < n[1])]
        src, dst = (1, 0) if (a, b) == REVERSED_PAIR else (0, 1)
        assert len(np.unique(m[:, src])) == len(m)
        m0 = np.full(n[src], -1, dtype=np.int16)
        m0[m[:, src]] = m[:, dst]
        names = (frame_name(b), frame_name(a)) if src else (frame_name(a), frame_name(b))
        formats.write_matches(store, formats.names_to_pair(*names), {"matches0": m0, "matching_scores0": np.ones(n[src], dtype=np.float16)})
        held.append((i, {tuple(r) for r in m.tolist()}))
    return store, held


def ring_scene(lengths=(2, 3, 17, 63, 64, 65), n_frames: int = 70, noise: float = 0.3, seed: int = 5) -> dict:
    """``n_frames`` frames on a ring around the origin; point p is seen by the first lengths[p] frames and matched along the chain
    (f, f + 1) and (f, f + 2): one track per point, of exactly that length."""
    key = ("ring", tuple(lengths), n_frames, noise, seed)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.RandomState(seed)
    ang = np.linspace(0.0, 2.0 * np.pi, n_frames, endpoint=False)
    centres = [np.array([9.0 * np.sin(a), 0.4 * np.sin(5 * a), -9.0 * np.cos(a)]) for a in ang]
    s = _base([CAMERAS[f % 5] for f in range(n_frames)], centres, [np.zeros(3)] * n_frames)
    xyz = rng.uniform(-1.0, 1.0, size=(len(lengths), 3))
    kps = [[] for _ in range(n_frames)]
    where = {}
    for f in range(n_frames):
        px, z = project(s, f, xyz)
        for p in rng.permutation(len(lengths)).tolist():
            if f < lengths[p]:
                assert z[p] > 0 and 0 <= px[p, 0] < WIDTH and 0 <= px[p, 1] < HEIGHT
                kps[f].append(tuple(px[p] - 0.5 + rng.uniform(-noise, noise, size=2)))
                where[(f, p)] = len(kps[f]) - 1
    pairs = [(f, f + d) for d in (1, 2) for f in range(n_frames - d)]
    matches = [[(where[(a, p)], where[(b, p)]) for p in range(len(lengths)) if (a, p) in where and (b, p) in where] for a, b in pairs]
    s.update(pairs=pairs, matches=matches, xyz=xyz, where=where, lengths=tuple(lengths), noise=noise)
    _scenes[key] = _finish(s, kps)
    return _scenes[key]
