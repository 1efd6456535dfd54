"""Numpy float64 restatement of the batched absolute-pose stage (csrc/pose.hip), for the tests of pram_amd.localization.pose.

Plain host code written from the algorithm of DESIGN.md 4.12: the counter-based sampler, Grunert's P3P quartic, the scoring and
ranking rule, the Levenberg-Marquardt refinement and the candidate selection.  It is NOT pycolmap (which the reference calls and
which is not available to these tests); it is the yardstick the device kernels are compared with, and tests/test_pose_cpu.py
checks it against itself and against scipy first.  Also the seeded scene builders the CPU and GPU tests share."""
from __future__ import annotations

import numpy as np

MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4}
N_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8}
UNDISTORT_STEPS = 10      # PRAM_POSE_UNDISTORT_STEPS
CUBIC_POLISH = 2          # Newton steps on the resolvent cubic's root
QUARTIC_POLISH = 3        # Newton steps on every root of the quartic
LM_LAMBDA0 = 1e-3
_IGN = dict(all="ignore")


# ---------------------------------------------------------------- cameras (COLMAP's models and parameter order)
def unify(model: int, params):
    """-> (fx, fy, cx, cy, k1, k2, p1, p2): every supported model is OPENCV with some coefficients zero."""
    p = [float(x) for x in params] + [0.0] * 8
    if model == 0:
        return p[0], p[0], p[1], p[2], 0.0, 0.0, 0.0, 0.0
    if model == 1:
        return p[0], p[1], p[2], p[3], 0.0, 0.0, 0.0, 0.0
    if model == 2:
        return p[0], p[0], p[1], p[2], p[3], 0.0, 0.0, 0.0
    if model == 3:
        return p[0], p[0], p[1], p[2], p[3], p[4], 0.0, 0.0
    if model == 4:
        return tuple(p[:8])
    raise ValueError(f"camera model {model}")


def camera_row(cam):
    """(model_name, width, height, params) -> (model id, params[8] zero padded)."""
    m = MODELS[cam[0]]
    p = np.zeros(8)
    p[:N_PARAMS[m]] = np.asarray(cam[3], dtype=np.float64)[:N_PARAMS[m]]
    return m, p


def distort(u, v, k1, k2, p1, p2):
    """COLMAP's distortion function, (u, v) normalised -> (u + du, v + dv)."""
    r2 = u * u + v * v
    rad = k1 * r2 + k2 * r2 * r2
    du = u * rad + 2.0 * p1 * u * v + p2 * (r2 + 2.0 * u * u)
    dv = v * rad + 2.0 * p2 * u * v + p1 * (r2 + 2.0 * v * v)
    return u + du, v + dv


def distort_jac(u, v, k1, k2, p1, p2):
    """d(distort) / d(u, v) -> j11, j12, j21, j22."""
    r2 = u * u + v * v
    rad = k1 * r2 + k2 * r2 * r2
    dr = k1 + 2.0 * k2 * r2
    j11 = 1.0 + rad + 2.0 * u * u * dr + 2.0 * p1 * v + 6.0 * p2 * u
    j12 = 2.0 * u * v * dr + 2.0 * p1 * u + 2.0 * p2 * v
    j21 = j12
    j22 = 1.0 + rad + 2.0 * v * v * dr + 2.0 * p2 * u + 6.0 * p1 * v
    return j11, j12, j21, j22


def undistort(xd, yd, k1, k2, p1, p2, steps: int = UNDISTORT_STEPS):
    """A fixed number of Newton steps on distort(u, v) = (xd, yd), started at (xd, yd)."""
    xd, yd = np.asarray(xd, dtype=np.float64), np.asarray(yd, dtype=np.float64)
    u, v = xd.copy(), yd.copy()
    with np.errstate(**_IGN):
        for _ in range(steps):
            fu, fv = distort(u, v, k1, k2, p1, p2)
            fu, fv = fu - xd, fv - yd
            j11, j12, j21, j22 = distort_jac(u, v, k1, k2, p1, p2)
            det = j11 * j22 - j12 * j21
            ok = np.abs(det) > 1e-12
            su = np.where(ok, (j22 * fu - j12 * fv) / det, 0.0)
            sv = np.where(ok, (j11 * fv - j21 * fu) / det, 0.0)
            u, v = u - su, v - sv
    return u, v


def prepare(kpts, model: int, params):
    """pram_pose_prepare: float32 keypoints [n, 2] -> normalised camera-plane points [n, 2] float64."""
    fx, fy, cx, cy, k1, k2, p1, p2 = unify(model, params)
    k = np.asarray(kpts, dtype=np.float32).astype(np.float64) + 0.5
    u, v = undistort((k[:, 0] - cx) / fx, (k[:, 1] - cy) / fy, k1, k2, p1, p2)
    return np.stack([u, v], 1)


def project(xyz, R, t, model: int, params):
    """World points -> pixels through the full camera model (and the depths)."""
    fx, fy, cx, cy, k1, k2, p1, p2 = unify(model, params)
    xc = xyz @ R.T + t
    u, v = distort(xc[:, 0] / xc[:, 2], xc[:, 1] / xc[:, 2], k1, k2, p1, p2)
    return np.stack([fx * u + cx, fy * v + cy], 1), xc[:, 2]


def f_mean(model: int, params) -> float:
    fx, fy = unify(model, params)[:2]
    return (fx + fy) / 2.0


# ---------------------------------------------------------------- the sampler (integer for integer what the device draws)
_U = np.uint64


def sm64(x):
    """splitmix64's output function of x + golden gamma, on uint64 arrays."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=_U) + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def draw_u64(seed: int, p: int, trial, draw: int):
    """The 64-bit word of (seed, pair, trial, draw): sm64(sm64(sm64(seed) ^ (p << 32 | trial)) + draw)."""
    trial = np.asarray(trial, dtype=_U)
    with np.errstate(over="ignore"):
        key = sm64(sm64(np.array([seed & 0xFFFFFFFFFFFFFFFF], dtype=_U)) ^ ((_U(p) << _U(32)) | trial))
        return sm64(key + _U(draw))


def mulhi(u, n: int):
    """floor(u * n / 2^64) for uint64 u and 0 <= n < 2^31, from 32-bit halves."""
    n = _U(n)
    return (((u >> _U(32)) * n + (((u & _U(0xFFFFFFFF)) * n) >> _U(32))) >> _U(32)).astype(np.int64)


def sample_triples(seed: int, p: int, n: int, trials: int) -> np.ndarray:
    """[trials, 3] distinct row indices below n (n >= 3): index k is drawn from [0, n - k) and stepped over the earlier ones."""
    tr = np.arange(trials)
    i0 = mulhi(draw_u64(seed, p, tr, 0), n)
    i1 = mulhi(draw_u64(seed, p, tr, 1), n - 1)
    i2 = mulhi(draw_u64(seed, p, tr, 2), n - 2)
    i1 = i1 + (i1 >= i0)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = i2 + (i2 >= lo)
    i2 = i2 + (i2 >= hi)
    return np.stack([i0, i1, i2], 1)


# ---------------------------------------------------------------- P3P: Grunert's quartic, vectorised over trials
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def quartic_roots(A4, A3, A2, A1, A0):
    """Real roots of A4 v^4 + .. + A0 (arrays over trials): Ferrari's closed form through the largest root of the resolvent cubic,
    then QUARTIC_POLISH Newton steps on the polynomial itself.  -> (roots [H, 4], valid [H, 4]), slots in the fixed order
    (first quadratic +, -, second quadratic +, -)."""
    with np.errstate(**_IGN):
        b, c, d, e = A3 / A4, A2 / A4, A1 / A4, A0 / A4
        p = c - 0.375 * b * b
        q = d - 0.5 * b * c + 0.125 * b * b * b
        r = e - 0.25 * b * d + 0.0625 * b * b * c - 0.01171875 * b * b * b * b
        a2, a1, a0 = p, 0.25 * (p * p - 4.0 * r), -0.125 * q * q
        Qc = (a2 * a2 - 3.0 * a1) / 9.0
        Rc = (2.0 * a2 * a2 * a2 - 9.0 * a2 * a1 + 27.0 * a0) / 54.0
        Q3 = Qc * Qc * Qc
        three = Rc * Rc < Q3
        th = np.arccos(np.clip(Rc / np.sqrt(np.where(three, Q3, 1.0)), -1.0, 1.0))
        sq = -2.0 * np.sqrt(np.where(three, Qc, 0.0))
        m3 = np.maximum(np.maximum(sq * np.cos(th / 3.0), sq * np.cos((th + 2.0 * np.pi) / 3.0)), sq * np.cos((th - 2.0 * np.pi) / 3.0))
        A = -np.sign(Rc) * np.cbrt(np.abs(Rc) + np.sqrt(np.where(three, 0.0, Rc * Rc - Q3)))
        B = np.where(A != 0.0, Qc / np.where(A != 0.0, A, 1.0), 0.0)
        m = np.where(three, m3, A + B) - a2 / 3.0
        for _ in range(CUBIC_POLISH):
            g = ((m + a2) * m + a1) * m + a0
            dg = (3.0 * m + 2.0 * a2) * m + a1
            m = np.where(dg != 0.0, m - g / np.where(dg != 0.0, dg, 1.0), m)
        main = m > 0.0
        s = np.sqrt(2.0 * np.where(main, m, 1.0))
        h = 0.5 * p + m
        g = q / (2.0 * s)
        d1, d2 = s * s - 4.0 * (h + g), s * s - 4.0 * (h - g)
        r1, r2 = np.sqrt(np.maximum(d1, 0.0)), np.sqrt(np.maximum(d2, 0.0))
        ym = np.stack([0.5 * (s + r1), 0.5 * (s - r1), 0.5 * (-s + r2), 0.5 * (-s - r2)], 1)
        vm = np.stack([d1 >= 0.0, d1 >= 0.0, d2 >= 0.0, d2 >= 0.0], 1)
        # q = 0 (the resolvent's largest root is not positive): a biquadratic, y^2 = (-p +- sqrt(p^2 - 4 r)) / 2
        db = p * p - 4.0 * r
        rb = np.sqrt(np.maximum(db, 0.0))
        z1, z2 = 0.5 * (-p + rb), 0.5 * (-p - rb)
        w1, w2 = np.sqrt(np.maximum(z1, 0.0)), np.sqrt(np.maximum(z2, 0.0))
        yb = np.stack([w1, -w1, w2, -w2], 1)
        ok1, ok2 = (db >= 0.0) & (z1 >= 0.0), (db >= 0.0) & (z2 >= 0.0)
        vb = np.stack([ok1, ok1, ok2, ok2], 1)
        y = np.where(main[:, None], ym, yb)
        valid = np.where(main[:, None], vm, vb)
        v = y - 0.25 * b[:, None]
        for _ in range(QUARTIC_POLISH):
            f = (((A4[:, None] * v + A3[:, None]) * v + A2[:, None]) * v + A1[:, None]) * v + A0[:, None]
            df = ((4.0 * A4[:, None] * v + 3.0 * A3[:, None]) * v + 2.0 * A2[:, None]) * v + A1[:, None]
            v = np.where(df != 0.0, v - f / np.where(df != 0.0, df, 1.0), v)
        valid = valid & np.isfinite(v)
    return v, valid


def p3p(x, X, return_diag: bool = False):
    """x [H, 3, 2] normalised image points, X [H, 3, 3] world points -> (poses [H, 4, 12] row-major R | t cam_from_world, the
    first n_sol[h] slots valid and the rest zero, n_sol [H]).  Grunert's formulation (Haralick et al., IJCV 1994): with the
    distances s2 = u s1, s3 = v s1 the law-of-cosines system is reduced to one quartic in v."""
    H = x.shape[0]
    with np.errstate(**_IGN):
        j = np.concatenate([x, np.ones((H, 3, 1))], 2)
        j = j / np.sqrt(x[:, :, 0] * x[:, :, 0] + x[:, :, 1] * x[:, :, 1] + 1.0)[:, :, None]
        P1, P2, P3 = X[:, 0], X[:, 1], X[:, 2]
        d12, d13, d23 = P2 - P1, P3 - P1, P3 - P2
        a2, b2, c2 = _dot(d23, d23), _dot(d13, d13), _dot(d12, d12)
        cr = _cross(d12, d13)
        cr2 = _dot(cr, cr)
        live = cr2 > 1e-18 * c2 * b2
        ca, cb, cg = _dot(j[:, 1], j[:, 2]), _dot(j[:, 0], j[:, 2]), _dot(j[:, 0], j[:, 1])
        K, cr_ = (a2 - c2) / b2, c2 / b2
        n2, n1, n0 = K - 1.0, -2.0 * K * cb, 1.0 + K
        e1, e0 = -2.0 * ca, 2.0 * cg
        q2, q1, q0 = -cr_, 2.0 * cr_ * cb, 1.0 - cr_
        dd2, dd1, dd0 = e1 * e1, 2.0 * e1 * e0, e0 * e0
        A4 = n2 * n2 + dd2 * q2
        A3 = 2.0 * n2 * n1 + (dd2 * q1 + dd1 * q2) - e0 * (n2 * e1)
        A2 = (2.0 * n2 * n0 + n1 * n1) + (dd2 * q0 + dd1 * q1 + dd0 * q2) - e0 * (n2 * e0 + n1 * e1)
        A1 = 2.0 * n1 * n0 + (dd1 * q0 + dd0 * q1) - e0 * (n1 * e0 + n0 * e1)
        A0 = n0 * n0 + dd0 * q0 - e0 * (n0 * e0)
        v, valid = quartic_roots(A4, A3, A2, A1, A0)
        Dv = e1[:, None] * v + e0[:, None]
        u = ((n2[:, None] * v + n1[:, None]) * v + n0[:, None]) / Dv
        den = (1.0 + v * v) - (2.0 * v) * cb[:, None]
        s1 = np.sqrt(b2[:, None] / den)
        s2, s3 = u * s1, v * s1
        valid = valid & live[:, None] & (v > 0.0) & (u > 0.0) & (den > 0.0) & np.isfinite(s1) & np.isfinite(s2) & np.isfinite(s3) & (s1 > 0.0)
        # absolute orientation from the three point pairs: an orthonormal frame on each side
        w1 = d12 / np.sqrt(c2)[:, None]
        w3 = cr / np.sqrt(cr2)[:, None]
        w2 = _cross(w3, w1)
        poses = np.zeros((H, 4, 12))
        for k in range(4):
            C1, C2, C3 = s1[:, k, None] * j[:, 0], s2[:, k, None] * j[:, 1], s3[:, k, None] * j[:, 2]
            g12, g13 = C2 - C1, C3 - C1
            f1 = g12 / np.sqrt(_dot(g12, g12))[:, None]
            fc = _cross(g12, g13)
            f3 = fc / np.sqrt(_dot(fc, fc))[:, None]
            f2 = _cross(f3, f1)
            R = f1[:, :, None] * w1[:, None, :] + f2[:, :, None] * w2[:, None, :] + f3[:, :, None] * w3[:, None, :]
            t = C1 - np.stack([_dot(R[:, 0], P1), _dot(R[:, 1], P1), _dot(R[:, 2], P1)], 1)
            poses[:, k] = np.concatenate([R[:, 0], t[:, 0:1], R[:, 1], t[:, 1:2], R[:, 2], t[:, 2:3]], 1)
        valid = valid & np.all(np.isfinite(poses), axis=2)
    # compact the valid slots to the front, keeping their order
    order = np.argsort(~valid, axis=1, kind="stable")
    poses = np.take_along_axis(poses, order[:, :, None], axis=1)
    n_sol = valid.sum(1).astype(np.int32)
    poses[np.arange(4)[None, :] >= n_sol[:, None]] = 0.0
    if return_diag:
        with np.errstate(**_IGN):
            # conditioning of every valid root: |f'(v)| * |v| / sum |A_i v^i| (small = a near-multiple root)
            df = ((4.0 * A4[:, None] * v + 3.0 * A3[:, None]) * v + 2.0 * A2[:, None]) * v + A1[:, None]
            mag = np.abs(A4[:, None] * v ** 4) + np.abs(A3[:, None] * v ** 3) + np.abs(A2[:, None] * v * v) + np.abs(A1[:, None] * v) + np.abs(A0[:, None])
            cond = np.where(valid, np.abs(df * v) / mag, np.inf)
        return poses, n_sol, cond.min(1)
    return poses, n_sol


def pose_12(pose):
    m = np.asarray(pose).reshape(3, 4)
    return m[:, :3].copy(), m[:, 3].copy()


# ---------------------------------------------------------------- scoring and ranking
def score(pts, xyz, poses, thr2: float, chunk: int = 256):
    """poses [M, 12] -> (inlier count [M] int32, sum of inlier squared residuals [M]) in the normalised plane; a point with
    non-positive depth is an outlier."""
    M = poses.shape[0]
    cnt, res = np.zeros(M, dtype=np.int32), np.zeros(M)
    with np.errstate(**_IGN):
        for a in range(0, M, chunk):
            ps = poses[a:a + chunk]
            X, Y, Z = xyz[None, :, 0], xyz[None, :, 1], xyz[None, :, 2]
            xc = ps[:, 0, None] * X + ps[:, 1, None] * Y + ps[:, 2, None] * Z + ps[:, 3, None]
            yc = ps[:, 4, None] * X + ps[:, 5, None] * Y + ps[:, 6, None] * Z + ps[:, 7, None]
            zc = ps[:, 8, None] * X + ps[:, 9, None] * Y + ps[:, 10, None] * Z + ps[:, 11, None]
            du, dv = xc / zc - pts[None, :, 0], yc / zc - pts[None, :, 1]
            e = du * du + dv * dv
            inl = (zc > 0.0) & (e <= thr2)
            cnt[a:a + chunk] = inl.sum(1)
            res[a:a + chunk] = np.where(inl, e, 0.0).sum(1)
    return cnt, res


def inlier_mask(pts, xyz, R, t, thr2: float):
    with np.errstate(**_IGN):
        xc = xyz @ R.T + t
        e = (xc[:, 0] / xc[:, 2] - pts[:, 0]) ** 2 + (xc[:, 1] / xc[:, 2] - pts[:, 1]) ** 2
        return (xc[:, 2] > 0.0) & (e <= thr2), e


def rank(cnt, res, valid) -> int:
    """The contract's order: most inliers, then smaller residual sum, then smaller index; -1 if no slot is valid."""
    idx = np.nonzero(valid)[0]
    if idx.size == 0:
        return -1
    return int(idx[np.lexsort((idx, res[idx], -cnt[idx].astype(np.int64)))[0]])


# ---------------------------------------------------------------- refinement
def rodrigues(w):
    th = float(np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]))
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    Kx = Kx / th
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def lm_pass(kpx, xyz, mask, R, t, cam8):
    """Cauchy cost (scale 1 px), J^T W J and J^T W r over the masked rows; residuals in pixels through the full model."""
    fx, fy, cx, cy, k1, k2, p1, p2 = cam8
    X = xyz[mask]
    with np.errstate(**_IGN):
        Y = X @ R.T
        xc = Y + t
        z = xc[:, 2]
        ok = z > 1e-12
        u, v = xc[:, 0] / z, xc[:, 1] / z
        ud, vd = distort(u, v, k1, k2, p1, p2)
        r = np.stack([fx * ud + cx - kpx[mask, 0], fy * vd + cy - kpx[mask, 1]], 1)
        j11, j12, j21, j22 = distort_jac(u, v, k1, k2, p1, p2)
        # A = diag(fx, fy) Jd [[1/z, 0, -u/z], [0, 1/z, -v/z]]
        iz = 1.0 / z
        A = np.zeros((X.shape[0], 2, 3))
        A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = fx * j11 * iz, fx * j12 * iz, -fx * (j11 * u + j12 * v) * iz
        A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = fy * j21 * iz, fy * j22 * iz, -fy * (j21 * u + j22 * v) * iz
        # d xc / d omega = -[Y]x, d xc / d t = I
        J = np.zeros((X.shape[0], 2, 6))
        J[:, :, 0] = A[:, :, 2] * Y[:, 1, None] - A[:, :, 1] * Y[:, 2, None]
        J[:, :, 1] = A[:, :, 0] * Y[:, 2, None] - A[:, :, 2] * Y[:, 0, None]
        J[:, :, 2] = A[:, :, 1] * Y[:, 0, None] - A[:, :, 0] * Y[:, 1, None]
        J[:, :, 3:] = A
        s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        w = 1.0 / (1.0 + s)
        ok = ok & np.isfinite(s)
        w = np.where(ok, w, 0.0)
        J, r = np.where(ok[:, None, None], J, 0.0), np.where(ok[:, None], r, 0.0)
        cost = float(np.sum(np.where(ok, np.log1p(np.where(ok, s, 0.0)), 0.0)))
        Hm = np.einsum("n,nki,nkj->ij", w, J, J)
        g = np.einsum("n,nki,nk->i", w, J, r)
    return cost, Hm, g


def chol_solve6(Hm, g, lam):
    """(H + lam diag(H)) x = -g by Cholesky; None when a pivot is not positive."""
    M = Hm + lam * np.diag(np.diag(Hm))
    L = np.zeros((6, 6))
    for i in range(6):
        for k in range(i + 1):
            s = M[i, k] - np.dot(L[i, :k], L[k, :k])
            if i == k:
                if not s > 0.0:
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, k] = s / L[k, k]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def refine(kpx, xyz, mask, R, t, cam8, iters: int):
    R, t = R.copy(), t.copy()
    lam = LM_LAMBDA0
    cost, Hm, g = lm_pass(kpx, xyz, mask, R, t, cam8)
    for _ in range(iters):
        d = chol_solve6(Hm, g, lam)
        if d is None:
            lam *= 10.0
            continue
        R1, t1 = rodrigues(d[:3]) @ R, t + d[3:]
        c1, H1, g1 = lm_pass(kpx, xyz, mask, R1, t1, cam8)
        if c1 < cost:
            R, t, cost, Hm, g = R1, t1, c1, H1, g1
            lam = max(lam * 0.1, 1e-15)
        else:
            lam *= 10.0
    return R, t


def rot_to_qvec(R):
    """(w, x, y, z), w >= 0 (Shepperd's branches)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = np.sqrt(tr + 1.0) * 2.0
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2.0
        q = np.array([(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s])
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2.0
        q = np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s])
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2.0
        q = np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s])
    q = q / np.sqrt(np.dot(q, q))
    return -q if q[0] < 0.0 else q


def qvec_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# ---------------------------------------------------------------- one pair, all stages
def hypotheses(pts, xyz, seed: int, p: int, trials: int, return_diag: bool = False):
    n = pts.shape[0]
    if n < 3:
        z = (np.zeros((trials, 4, 12)), np.zeros(trials, dtype=np.int32))
        return z + (np.full(trials, np.inf),) if return_diag else z
    tri = sample_triples(seed, p, n, trials)
    return p3p(pts[tri], xyz[tri], return_diag)


def estimate_pose(kpts, xyz, cam, *, threshold: float, trials: int = 1000, min_inlier_ratio: float = 0.01, refine_iters: int = 20,
                  seed: int = 0, p: int = 0) -> dict:
    """The whole stage for pair p: kpts float32 [n, 2] (pixels, without the + 0.5), xyz float64 [n, 3], cam = (model_name, width,
    height, params).  -> dict(success, qvec, tvec, inliers [n] bool, num_inliers, best, n0)."""
    model, params = camera_row(cam)
    cam8 = unify(model, params)
    n = int(np.asarray(kpts).shape[0])
    fail = {"success": False, "qvec": np.zeros(4), "tvec": np.zeros(3), "inliers": np.zeros(n, dtype=bool), "num_inliers": 0, "best": -1, "n0": 0}
    if n < 3:
        return fail
    xyz = np.asarray(xyz, dtype=np.float64)
    pts = prepare(kpts, model, params)
    kpx = np.asarray(kpts, dtype=np.float32).astype(np.float64) + 0.5
    th = threshold / f_mean(model, params)
    thr2 = th * th
    poses, n_sol = hypotheses(pts, xyz, seed, p, trials)
    flat = poses.reshape(-1, 12)
    valid = (np.arange(4)[None, :] < n_sol[:, None]).reshape(-1)
    cnt, res = score(pts, xyz, flat, thr2)
    best = rank(cnt, res, valid)
    if best < 0:
        return fail
    n0 = int(cnt[best])
    fail["best"], fail["n0"] = best, n0
    if n0 < 3 or n0 < min_inlier_ratio * n:
        return fail
    R0, t0 = pose_12(flat[best])
    m0, _ = inlier_mask(pts, xyz, R0, t0, thr2)
    R1, t1 = refine(kpx, xyz, m0, R0, t0, cam8, refine_iters)
    m1, _ = inlier_mask(pts, xyz, R1, t1, thr2)
    R2, t2 = refine(kpx, xyz, m1, R1, t1, cam8, refine_iters)
    m2, _ = inlier_mask(pts, xyz, R2, t2, thr2)
    refined = True
    if int(m2.sum()) < n0 or not (np.all(np.isfinite(R2)) and np.all(np.isfinite(t2))):
        R2, t2, m2, refined = R0, t0, m0, False
    return {"success": True, "refined": refined, "qvec": rot_to_qvec(R2), "tvec": t2, "inliers": m2, "num_inliers": int(m2.sum()), "best": best, "n0": n0,
            "R": R2}


def select(success, num_inliers, min_inliers: int):
    """The reference's loop with verify_and_update and its early exit, for one query: -> (chosen candidate or -1, tracking
    status 1 / 0 / -1 (none), order of the chosen candidate or -1)."""
    kept, status = -1, -1
    for w in range(len(success)):
        if not success[w]:
            continue
        if kept < 0 or num_inliers[kept] < num_inliers[w]:
            kept = w
        if num_inliers[w] < min_inliers:
            status = 0
            continue
        status = 1
        break
    return kept, status, kept


# ---------------------------------------------------------------- seeded scenes
SCENE_CAMERAS = {
    "SIMPLE_PINHOLE": ("SIMPLE_PINHOLE", 640, 480, [520.0, 320.0, 240.0]),
    "PINHOLE": ("PINHOLE", 800, 600, [610.0, 590.0, 402.0, 297.0]),
    "SIMPLE_RADIAL": ("SIMPLE_RADIAL", 640, 480, [500.0, 318.0, 242.0, -0.08]),
    "RADIAL": ("RADIAL", 1024, 768, [820.0, 510.0, 380.0, -0.12, 0.03]),
    "OPENCV": ("OPENCV", 1280, 720, [900.0, 915.0, 642.0, 356.0, -0.10, 0.04, 0.001, -0.0008]),
}


def random_rotation(rng):
    q = rng.standard_normal(4)
    return qvec_to_rot(q / np.linalg.norm(q))


def make_scene(seed: int, cam, n: int, outlier_share: float, noise_px: float = 1.0, centre=(120.0, -340.0, 35.0)) -> dict:
    """A planted pose, n world points in front of the camera (a few hundred metres from the origin) projected through the camera
    model, Gaussian pixel noise, and a share of rows whose keypoint is replaced by a uniform one.  Keypoints are stored the way
    the matcher hands them over: float32 pixels without the + 0.5."""
    rng = np.random.default_rng(seed)
    model, params = camera_row(cam)
    w, h = cam[1], cam[2]
    fx, fy, cx, cy = unify(model, params)[:4]
    R = random_rotation(rng)
    # camera-frame points inside the image, 3 .. 30 m deep
    u = rng.uniform(0.05 * w, 0.95 * w, n)
    v = rng.uniform(0.05 * h, 0.95 * h, n)
    z = rng.uniform(3.0, 30.0, n)
    xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    t = -R @ np.asarray(centre) + rng.standard_normal(3)
    xyz = (xc - t) @ R      # R^T (xc - t)
    px, _ = project(xyz, R, t, model, params)
    px = px + noise_px * rng.standard_normal((n, 2))
    n_out = int(round(outlier_share * n))
    out_rows = rng.permutation(n)[:n_out]
    px[out_rows] = np.stack([rng.uniform(0, w, n_out), rng.uniform(0, h, n_out)], 1)
    is_out = np.zeros(n, dtype=bool)
    is_out[out_rows] = True
    return {"kpts": (px - 0.5).astype(np.float32), "xyz": np.ascontiguousarray(xyz), "R": R, "t": t, "cam": cam, "outlier": is_out, "n": n}


def pose_errors(R, t, R_gt, t_gt):
    """(rotation error in degrees, camera-centre error in metres)."""
    c = np.clip((np.trace(R @ R_gt.T) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(-R.T @ t + R_gt.T @ t_gt))


def pad_batch(scenes, t0: int = None):
    """Scenes -> the padded arrays pram_cand_correspond would have left: kpts [P, t0, 2] float32, xyz [P, t0, 3], counts [P]."""
    t0 = t0 or max(1, max(s["n"] for s in scenes))
    P = len(scenes)
    k, x, c = np.zeros((P, t0, 2), dtype=np.float32), np.zeros((P, t0, 3)), np.zeros(P, dtype=np.int32)
    for i, s in enumerate(scenes):
        k[i, :s["n"]], x[i, :s["n"]], c[i] = s["kpts"], s["xyz"], s["n"]
    return k, x, c


E2E_THRESHOLD = 4.0
E2E_COUNTS = {0.3: (12, 257, 2048, 64, 1000), 0.5: (40, 500, 33, 1500, 150), 0.7: (2048, 700, 90, 300, 100)}


def e2e_scenes(seed: int = 100):
    """Outlier shares 0.3, 0.5, 0.7 x the five camera models, 1 px noise, ragged counts from 12 to 2048: 15 pairs for one call
    (seg_k = 1, one camera per pair)."""
    out = []
    for share, counts in E2E_COUNTS.items():
        for (name, cam), n in zip(SCENE_CAMERAS.items(), counts):
            out.append(make_scene(seed + len(out), cam, n, share))
    return out


def scipy_refine(scene, mask, R, t):
    """An independent minimiser of the SAME cost as the restatement and the kernel: scipy.optimize.minimize (BFGS, numerical
    gradient) on sum_i log(1 + |r_i|^2), r_i the pixel residual of point i through the full camera model, over a left axis-angle
    increment and a translation increment, started at (R, t) and restarted until the cost stops falling.
    (least_squares(loss='cauchy') applies rho per scalar residual, i.e. per pixel coordinate: a different objective.)"""
    from scipy.optimize import minimize
    model, params = camera_row(scene["cam"])
    kpx = scene["kpts"].astype(np.float64) + 0.5
    xyz = scene["xyz"][mask]
    # parameters scaled so that a unit step moves a pixel by about a pixel: radians / f, metres / (f / depth)
    f = f_mean(model, params)
    sc = np.array([1.0 / f] * 3 + [10.0 / f] * 3)

    def cost(x, R0, t0):
        x = x * sc
        px, _ = project(xyz, rodrigues(x[:3]) @ R0, t0 + x[3:], model, params)
        d = px - kpx[mask]
        return float(np.sum(np.log1p(d[:, 0] ** 2 + d[:, 1] ** 2)))

    last = np.inf
    for _ in range(6):
        sol = minimize(cost, np.zeros(6), args=(R, t), method="BFGS", options={"gtol": 1e-10, "maxiter": 500})
        x = sol.x * sc
        R, t = rodrigues(x[:3]) @ R, t + x[3:]
        if not sol.fun < last - 1e-12 * abs(last):
            break
        last = sol.fun
    return R, t


# ---------------------------------------------------------------- the candidate tests' synthetic map with planted cameras
PLANTED_CAMERAS = (("SIMPLE_RADIAL", 640, 480, [520.0, 318.0, 242.0, -0.06]), ("PINHOLE", 640, 480, [505.0, 498.0, 322.0, 237.0]),
                   ("OPENCV", 640, 480, [540.0, 548.0, 316.0, 244.0, -0.08, 0.03, 0.0008, -0.0006]),
                   ("SIMPLE_PINHOLE", 640, 480, [515.0, 320.0, 240.0]), ("RADIAL", 640, 480, [530.0, 321.0, 239.0, -0.07, 0.02]))


def plant_cameras(map_: dict, queries, seed: int = 0, noise_px: float = 0.5):
    """tests/cand_ref.py's map and queries (make_map / make_query) made consistent with one planted camera per query: query b gets
    camera PLANTED_CAMERAS[b % 5] and a random pose, and every reference row that one of its keypoints is twinned from (query['twin'] =
    (frame, row)) gets the xyz that projects to that keypoint (+ 0.5, plus Gaussian noise) at a depth of 3 .. 30 m.  A row twinned by
    several queries belongs to the first; for the later ones it is an outlier, like every row that is nobody's twin (those keep the
    map's random xyz).  Changes map_['frames'][f]['xyzs'] in place.  -> per query dict(cam, R, t)."""
    rng = np.random.default_rng(seed)
    claimed = set()
    out = []
    for b, q in enumerate(queries):
        cam = PLANTED_CAMERAS[b % len(PLANTED_CAMERAS)]
        model, params = camera_row(cam)
        c = unify(model, params)
        R = random_rotation(rng)
        t = -R @ np.array([150.0 * (b + 1), -220.0, 40.0]) + rng.standard_normal(3)
        n = q["count"]
        px = q["keypoints"][:n].astype(np.float64) + 0.5 + noise_px * rng.standard_normal((n, 2))
        u, v = undistort((px[:, 0] - c[2]) / c[0], (px[:, 1] - c[3]) / c[1], *c[4:])
        z = rng.uniform(3.0, 30.0, n)
        xyz = (np.stack([u * z, v * z, z], 1) - t) @ R
        for i in range(n):
            f, row = int(q["twin"][i, 0]), int(q["twin"][i, 1])
            if f < 0 or (f, row) in claimed:
                continue
            claimed.add((f, row))
            map_["frames"][f]["xyzs"][row] = xyz[i]
        out.append({"cam": cam, "R": R, "t": t})
    return out
