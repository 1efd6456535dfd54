"""numpy restatement of csrc/twoview.hip in the kernel's order of operations: the five-point sampler, the five-point solver (null
space by complete pivoting, the ten cubic constraints, elimination, the degree-10 polynomial of the hidden variable z, Sturm
bisection, Newton on det B(z)), Sampson scoring, the ranking rule, the decomposition, the 5-DoF Levenberg-Marquardt and the success
rule.  Also the planted two-view scenes the tests share.  DESIGN.md 4.24 has the formulas."""
from __future__ import annotations

import numpy as np

from tests import pose_ref as PR

MAX_SOL = 10
BISECT = 48           # bisection steps per root on the Sturm count
NEWTON = 4            # Newton steps per root on det B(z)
CHECK_TOL = 1e-6      # a root is kept when |det E| and every entry of 2 E E^T E - tr(E E^T) E stay below it (|E|_F = 1)
RANK_EPS = 1e-10      # a pivot of the 5 x 9 system below RANK_EPS * the first pivot: rank-deficient
LM_LAMBDA0 = 1e-3
DEFAULTS = dict(max_error=4.0, trials=1024, seed=0, min_inlier_ratio=0.1, min_num_inliers=15, refine_iters=20, pair_chunk=256)
_IGN = dict(all="ignore")

# ---------------------------------------------------------------- monomial tables (the kernel holds the same, as literals)
MON1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]                                              # x, y, z, 1
MON2 = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
# Nister's column order: the ten monomials that are eliminated, then x z^2, x z, x, y z^2, y z, y, z^3, z^2, z, 1
MON3 = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
        (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


T11 = np.array([[MON2.index(_add(a, b)) for b in MON1] for a in MON1])      # [4][4] -> index among MON2
T21 = np.array([[MON3.index(_add(a, b)) for b in MON1] for a in MON2])      # [10][4] -> index among MON3


def mul11(a, b):
    """degree-1 x degree-1 polynomials [..., 4] -> [..., 10]"""
    out = np.zeros(a.shape[:-1] + (10,))
    for i in range(4):
        for j in range(4):
            out[..., T11[i, j]] += a[..., i] * b[..., j]
    return out


def mul21(a, b):
    """degree-2 x degree-1 polynomials [..., 10], [..., 4] -> [..., 20]"""
    out = np.zeros(a.shape[:-1] + (20,))
    for i in range(10):
        for j in range(4):
            out[..., T21[i, j]] += a[..., i] * b[..., j]
    return out


# ---------------------------------------------------------------- the sampler
def sample_fives(seed: int, p: int, n: int, trials: int) -> np.ndarray:
    """[trials, 5] distinct indices below n: pick k is drawn from [0, n - k) and stepped over the earlier picks in ascending
    order.  All -1 when n < 5."""
    if n < 5:
        return np.full((trials, 5), -1, dtype=np.int64)
    tr = np.arange(trials)
    picks = np.zeros((trials, 5), dtype=np.int64)
    for k in range(5):
        i = PR.mulhi(PR.draw_u64(seed, p, tr, k), n - k)
        earlier = np.sort(picks[:, :k], axis=1)
        for j in range(k):
            i = i + (i >= earlier[:, j])
        picks[:, k] = i
    return picks


# ---------------------------------------------------------------- the five-point solver, vectorised over trials
def null_space(A):
    """A [T, 5, 9] -> (basis [T, 4, 9], ok [T]): Gauss-Jordan with complete pivoting (first maximum in row-major order)."""
    A = A.copy()
    T = A.shape[0]
    ar = np.arange(T)
    perm = np.tile(np.arange(9), (T, 1))
    ok = np.ones(T, dtype=bool)
    first = None
    with np.errstate(**_IGN):
        for k in range(5):
            sub = np.abs(A[:, k:, k:]).reshape(T, -1)
            sub = np.where(np.isnan(sub), -1.0, sub)
            flat = np.argmax(sub, axis=1)
            r, c = k + flat // (9 - k), k + flat % (9 - k)
            piv = sub[ar, flat]
            first = piv if k == 0 else first
            ok &= piv > RANK_EPS * first
            tmp = A[ar, k].copy(); A[ar, k] = A[ar, r]; A[ar, r] = tmp
            tmp = A[ar, :, k].copy(); A[ar, :, k] = A[ar, :, c]; A[ar, :, c] = tmp
            tmp = perm[ar, k].copy(); perm[ar, k] = perm[ar, c]; perm[ar, c] = tmp
            A[:, k] = A[:, k] / A[:, k, k][:, None]
            for i in range(5):
                if i != k:
                    A[:, i] = A[:, i] - A[:, i, k][:, None] * A[:, k]
    basis = np.zeros((T, 4, 9))
    for j in range(4):
        basis[ar, j, perm[:, 5 + j]] = 1.0
        for i in range(5):
            basis[ar, j, perm[:, i]] = -A[:, i, 5 + j]
    return basis, ok


def constraints(basis):
    """basis [T, 4, 9] (X, Y, Z, W) -> the 10 x 20 matrix [T, 10, 20]: det E, then the nine entries of (E E^T - tr / 2) E."""
    e = np.transpose(basis, (0, 2, 1))      # [T, 9, 4]: entry ij as a polynomial in (x, y, z, 1)
    E = lambda i, j: e[:, 3 * i + j]
    M = np.zeros((basis.shape[0], 10, 20))
    M[:, 0] = (mul21(mul11(E(1, 1), E(2, 2)) - mul11(E(1, 2), E(2, 1)), E(0, 0)) - mul21(mul11(E(1, 0), E(2, 2)) - mul11(E(1, 2), E(2, 0)), E(0, 1))
               + mul21(mul11(E(1, 0), E(2, 1)) - mul11(E(1, 1), E(2, 0)), E(0, 2)))
    G = [[(mul11(E(i, 0), E(j, 0)) + mul11(E(i, 1), E(j, 1))) + mul11(E(i, 2), E(j, 2)) for j in range(3)] for i in range(3)]
    half = 0.5 * ((G[0][0] + G[1][1]) + G[2][2])
    for i in range(3):
        G[i][i] = G[i][i] - half
    for i in range(3):
        for j in range(3):
            M[:, 1 + 3 * i + j] = (mul21(G[i][0], E(0, j)) + mul21(G[i][1], E(1, j))) + mul21(G[i][2], E(2, j))
    return M


def eliminate(M):
    """Gauss-Jordan with partial pivoting over the first ten columns -> (M, ok)."""
    M = M.copy()
    T = M.shape[0]
    ar = np.arange(T)
    ok = np.ones(T, dtype=bool)
    with np.errstate(**_IGN):
        for k in range(10):
            col = np.abs(M[:, k:, k])
            col = np.where(np.isnan(col), -1.0, col)
            r = k + np.argmax(col, axis=1)
            ok &= col[ar, r - k] > 1e-300
            tmp = M[ar, k].copy(); M[ar, k] = M[ar, r]; M[ar, r] = tmp
            M[:, k] = M[:, k] / M[:, k, k][:, None]
            for i in range(10):
                if i != k:
                    M[:, i] = M[:, i] - M[:, i, k][:, None] * M[:, k]
    return M, ok


def hidden_matrix(M):
    """rows (4, 5), (6, 7), (8, 9) of the eliminated system -> B [T, 3, 13]: per row p (4 ascending coefficients in z), q (4), r (5)
    of  x p(z) + y q(z) + r(z) = 0."""
    T = M.shape[0]
    B = np.zeros((T, 3, 13))
    for k in range(3):
        a, b = M[:, 4 + 2 * k, 10:], M[:, 5 + 2 * k, 10:]
        B[:, k, 0], B[:, k, 1], B[:, k, 2], B[:, k, 3] = a[:, 2], a[:, 1] - b[:, 2], a[:, 0] - b[:, 1], -b[:, 0]
        B[:, k, 4], B[:, k, 5], B[:, k, 6], B[:, k, 7] = a[:, 5], a[:, 4] - b[:, 5], a[:, 3] - b[:, 4], -b[:, 3]
        B[:, k, 8], B[:, k, 9], B[:, k, 10], B[:, k, 11], B[:, k, 12] = a[:, 9], a[:, 8] - b[:, 9], a[:, 7] - b[:, 8], a[:, 6] - b[:, 7], -b[:, 6]
    return B


def _conv(a, b):
    out = np.zeros((a.shape[0], a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            out[:, i + j] += a[:, i] * b[:, j]
    return out


def det_poly(B):
    """det B(z) -> [T, 11] ascending."""
    p, q, r = B[:, :, 0:4], B[:, :, 4:8], B[:, :, 8:13]
    m0 = _conv(q[:, 1], r[:, 2]) - _conv(q[:, 2], r[:, 1])      # degree 7
    m1 = _conv(p[:, 1], r[:, 2]) - _conv(p[:, 2], r[:, 1])      # degree 7
    m2 = _conv(p[:, 1], q[:, 2]) - _conv(p[:, 2], q[:, 1])      # degree 6
    return (_conv(p[:, 0], m0) - _conv(q[:, 0], m1)) + _conv(r[:, 0], m2)


def _horner(c, x, deg):
    v = c[:, deg]
    for i in range(deg - 1, -1, -1):
        v = v * x + c[:, i]
    return v


def sturm_chain(c):
    """c [T, 11] -> S [T, 11, 11]: S[i] of degree 10 - i, every remainder divided by its largest magnitude."""
    T = c.shape[0]
    S = np.zeros((T, 11, 11))
    with np.errstate(**_IGN):
        S[:, 0] = c
        for i in range(1, 11):
            S[:, 1, i - 1] = i * c[:, i]
        for k in range(1, 10):
            n = 11 - k      # degree of S[k - 1]; S[k] has n - 1
            a, b = S[:, k - 1], S[:, k]
            q1 = a[:, n] / b[:, n - 1]
            q0 = (a[:, n - 1] - q1 * b[:, n - 2]) / b[:, n - 1]
            r = np.zeros((T, 11))
            for i in range(n - 1):
                r[:, i] = (a[:, i] - (q1 * b[:, i - 1] if i > 0 else 0.0)) - q0 * b[:, i]
            s = np.max(np.abs(r[:, :n - 1]), axis=1)
            S[:, k + 1] = -r / s[:, None]
    return S


def sign_changes(S, x):
    cnt = np.zeros(S.shape[0], dtype=np.int64)
    last = np.zeros(S.shape[0], dtype=np.int64)
    with np.errstate(**_IGN):
        for i in range(11):
            v = _horner(S[:, i], x, 10 - i)
            sg = np.where(v > 0.0, 1, np.where(v < 0.0, -1, 0))
            cnt += (sg != 0) & (last != 0) & (sg != last)
            last = np.where(sg != 0, sg, last)
    return cnt


def _det3(a, b, c):
    return (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0])) + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])


def _rows_at(B, z):
    """B(z) and B'(z): two lists of three [T, 3] rows"""
    val, der = [], []
    for k in range(3):
        v, d = [], []
        for lo, deg in ((0, 3), (4, 3), (8, 4)):
            c = B[:, k, lo:lo + deg + 1]
            v.append(_horner(c, z, deg))
            dv = deg * c[:, deg]
            for i in range(deg - 1, 0, -1):
                dv = dv * z + i * c[:, i]
            d.append(dv)
        val.append(np.stack(v, 1))
        der.append(np.stack(d, 1))
    return val, der


def violation(E):
    """E [T, 9] -> the largest magnitude among det E and the nine entries of 2 E E^T E - tr(E E^T) E"""
    e = [E[:, i] for i in range(9)]
    with np.errstate(**_IGN):
        det = (e[0] * (e[4] * e[8] - e[5] * e[7]) - e[1] * (e[3] * e[8] - e[5] * e[6])) + e[2] * (e[3] * e[7] - e[4] * e[6])
        G = [[(e[3 * i] * e[3 * j] + e[3 * i + 1] * e[3 * j + 1]) + e[3 * i + 2] * e[3 * j + 2] for j in range(3)] for i in range(3)]
        tr = (G[0][0] + G[1][1]) + G[2][2]
        worst = np.abs(det)
        for i in range(3):
            for j in range(3):
                c = 2.0 * ((G[i][0] * e[j] + G[i][1] * e[3 + j]) + G[i][2] * e[6 + j]) - tr * e[3 * i + j]
                worst = np.maximum(worst, np.abs(c))
    return np.where(np.isnan(worst), np.inf, worst)


def five_point(x0, x1, return_diag: bool = False):
    """x0, x1 [T, 5, 2]: normalised points of frame 0 and frame 1 -> (E [T, 10, 9] Frobenius-normalised, valid ones first in
    ascending z, zeros behind; n_sol [T])."""
    T = x0.shape[0]
    h0 = np.concatenate([x0, np.ones((T, 5, 1))], 2)
    h1 = np.concatenate([x1, np.ones((T, 5, 1))], 2)
    A = (h1[:, :, :, None] * h0[:, :, None, :]).reshape(T, 5, 9)      # x1^T E x0 = 0, E row-major
    basis, ok = null_space(A)
    M, ok2 = eliminate(constraints(basis))
    ok &= ok2
    B = hidden_matrix(M)
    with np.errstate(**_IGN):
        c = det_poly(B)
        c = c / np.max(np.abs(c), axis=1)[:, None]
        bound = 1.0 + np.max(np.abs(c[:, :10] / c[:, 10:11]), axis=1)
        S = sturm_chain(c)
        ok &= np.isfinite(bound) & np.isfinite(S).all(axis=(1, 2))
        bound = np.where(ok, bound, 1.0)
        S = np.where(ok[:, None, None], S, 0.0)
        v_lo = sign_changes(S, -bound)
        n_roots = np.clip(v_lo - sign_changes(S, bound), 0, MAX_SOL)
        n_roots = np.where(ok, n_roots, 0)
        out = np.zeros((T, MAX_SOL, 9))
        n_sol = np.zeros(T, dtype=np.int32)
        ar = np.arange(T)
        for k in range(1, MAX_SOL + 1):
            lo, hi = -bound, bound.copy()
            for _ in range(BISECT):
                mid = 0.5 * (lo + hi)
                ge = (v_lo - sign_changes(S, mid)) >= k
                hi = np.where(ge, mid, hi)
                lo = np.where(ge, lo, mid)
            z = 0.5 * (lo + hi)
            for _ in range(NEWTON):
                val, der = _rows_at(B, z)
                f = _det3(val[0], val[1], val[2])
                df = (_det3(der[0], val[1], val[2]) + _det3(val[0], der[1], val[2])) + _det3(val[0], val[1], der[2])
                step = f / df
                z = np.where(np.isfinite(step), z - step, z)
            val, _ = _rows_at(B, z)
            best, bn = None, None
            for i, j in ((0, 1), (0, 2), (1, 2)):      # the null vector of B(z): the largest of the three cross products
                cr = PR._cross(val[i], val[j])
                nn = PR._dot(cr, cr)
                if best is None:
                    best, bn = cr, nn
                else:
                    take = nn > bn
                    best, bn = np.where(take[:, None], cr, best), np.where(take, nn, bn)
            x, y = best[:, 0] / best[:, 2], best[:, 1] / best[:, 2]
            E = ((x[:, None] * basis[:, 0] + y[:, None] * basis[:, 1]) + z[:, None] * basis[:, 2]) + basis[:, 3]
            nrm = np.sqrt(np.sum(E * E, axis=1))
            E = E / nrm[:, None]
            good = (k <= n_roots) & np.isfinite(E).all(axis=1) & (nrm > 0.0) & (violation(E) <= CHECK_TOL)
            out[ar[good], n_sol[good]] = E[good]
            n_sol[good] += 1
    if return_diag:
        return out, n_sol, {"basis": basis, "M": M, "poly": c}
    return out, n_sol


def pair_rows(norm, frame_off, f0: int, f1: int, matches):
    """The rows of a pair as the kernels read them: [n, 4] (u0, v0, u1, v1), NaN where an index is outside its frame."""
    m = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
    r0, n0, r1, n1 = frame_off[f0], frame_off[f0 + 1] - frame_off[f0], frame_off[f1], frame_off[f1 + 1] - frame_off[f1]
    ok = (m[:, 0] >= 0) & (m[:, 0] < n0) & (m[:, 1] >= 0) & (m[:, 1] < n1)
    rows = np.full((m.shape[0], 4), np.nan)
    rows[ok, 0:2] = norm[r0 + m[ok, 0]]
    rows[ok, 2:4] = norm[r1 + m[ok, 1]]
    return rows


def hypotheses(rows, seed: int, p: int, trials: int):
    """-> (E [trials, 10, 9], n_sol [trials], fives [trials, 5])"""
    n = rows.shape[0]
    fives = sample_fives(seed, p, n, trials)
    if n < 5:
        return np.zeros((trials, MAX_SOL, 9)), np.zeros(trials, dtype=np.int32), fives
    s = rows[fives]
    bad = ~np.isfinite(s).all(axis=(1, 2))
    s = np.where(bad[:, None, None], 0.0, s)
    E, n_sol = five_point(s[:, :, 0:2], s[:, :, 2:4])
    E[bad], n_sol[bad] = 0.0, 0
    return E, n_sol, fives


# ---------------------------------------------------------------- scoring
def sampson(E, rows):
    """E [H, 9], rows [n, 4] -> squared Sampson error [H, n] on the normalised plane, in the kernel's order"""
    u0, v0, u1, v1 = (rows[None, :, i] for i in range(4))
    e = [E[:, i, None] for i in range(9)]
    with np.errstate(**_IGN):
        a0, a1, a2 = (e[0] * u0 + e[1] * v0) + e[2], (e[3] * u0 + e[4] * v0) + e[5], (e[6] * u0 + e[7] * v0) + e[8]
        b0, b1 = (e[0] * u1 + e[3] * v1) + e[6], (e[1] * u1 + e[4] * v1) + e[7]
        c = (u1 * a0 + v1 * a1) + a2
        den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1
        return (c * c) / den


def threshold2(max_error: float, f0: float, f1: float) -> float:
    th = max_error * 0.5 * (1.0 / f0 + 1.0 / f1)
    return th * th


def score(E, n_sol, rows, thr2: float, chunk: int = 64):
    """E [T, 10, 9] -> (cnt [T * 10] int, -1 for an empty slot; res [T * 10])"""
    flat = E.reshape(-1, 9)
    cnt, res = np.zeros(flat.shape[0], dtype=np.int64), np.zeros(flat.shape[0])
    for a in range(0, flat.shape[0], chunk):
        e = sampson(flat[a:a + chunk], rows)
        with np.errstate(**_IGN):
            inl = e <= thr2
        cnt[a:a + chunk] = inl.sum(1)
        res[a:a + chunk] = np.where(inl, e, 0.0).sum(1)
    valid = (np.arange(MAX_SOL)[None, :] < n_sol[:, None]).reshape(-1)
    return np.where(valid, cnt, -1), np.where(valid, res, 0.0)


# ---------------------------------------------------------------- decomposition
def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def decompose(E9):
    """Frobenius-normalised E [9] -> four (R, t): (Ra, t), (Ra, -t), (Rb, t), (Rb, -t).  t: the largest cross product of two
    columns of E, normalised; R = cof(E') -+ [t]x E' with E' = sqrt(2) E (Horn 1990), then Gram-Schmidt with the third row
    the cross product of the first two, so det R = +1."""
    E = np.asarray(E9, dtype=np.float64).reshape(3, 3)
    cols = [E[:, 0], E[:, 1], E[:, 2]]
    best, bn = None, -1.0
    for i, j in ((0, 1), (0, 2), (1, 2)):
        cr = np.cross(cols[i], cols[j])
        nn = float(cr @ cr)
        if nn > bn:
            best, bn = cr, nn
    with np.errstate(**_IGN):
        t = best / np.sqrt(bn)
    Es = E * np.sqrt(2.0)
    cof = np.array([np.cross(Es[1], Es[2]), np.cross(Es[2], Es[0]), np.cross(Es[0], Es[1])])
    tE = _skew(t) @ Es
    out = []
    for R in (cof - tE, cof + tE):
        with np.errstate(**_IGN):
            r0 = R[0] / np.sqrt(R[0] @ R[0])
            r1 = R[1] - (R[1] @ r0) * r0
            r1 = r1 / np.sqrt(r1 @ r1)
        R = np.stack([r0, r1, np.cross(r0, r1)])
        out += [(R, t), (R, -t)]
    return out


def front_mask(R, t, rows):
    """rows at positive depth in both frames: lam0 from x1 x (lam0 R x0 + t) = 0, lam1 = (lam0 R x0 + t) . x1 / |x1|^2"""
    n = rows.shape[0]
    x0 = np.concatenate([rows[:, 0:2], np.ones((n, 1))], 1)
    x1 = np.concatenate([rows[:, 2:4], np.ones((n, 1))], 1)
    with np.errstate(**_IGN):
        y = x0 @ R.T
        a, b = np.cross(x1, y), np.cross(x1, np.broadcast_to(t, (n, 3)))
        lam0 = -np.sum(a * b, 1) / np.sum(a * a, 1)
        lam1 = np.sum((lam0[:, None] * y + t) * x1, 1) / np.sum(x1 * x1, 1)
        return (lam0 > 0.0) & (lam1 > 0.0)


def essential_of(R, t):
    return (_skew(t) @ R).reshape(9) / np.sqrt(2.0)


# ---------------------------------------------------------------- refinement: 5 degrees of freedom, Cauchy over Sampson distances
def tangent_basis(t):
    a = int(np.argmin(np.abs(t)))
    e = np.zeros(3)
    e[a] = 1.0
    b1 = np.cross(t, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return b1, np.cross(t, b1)


def lm_pass(rows, mask, R, t, scale: float):
    """cost, H [5, 5], g [5] of sum log(1 + (d / scale)^2), d the signed Sampson distance, over the masked rows"""
    r = rows[mask]
    n = r.shape[0]
    x0 = np.concatenate([r[:, 0:2], np.ones((n, 1))], 1)
    x1 = np.concatenate([r[:, 2:4], np.ones((n, 1))], 1)
    b1, b2 = tangent_basis(t)
    E = _skew(t) @ R
    dE = [_skew(t) @ _skew(np.eye(3)[k]) @ R for k in range(3)] + [_skew(b1) @ R, _skew(b2) @ R]
    with np.errstate(**_IGN):
        a, b = x0 @ E.T, x1 @ E
        c = np.sum(x1 * a, 1)
        den = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + b[:, 0] * b[:, 0]) + b[:, 1] * b[:, 1]
        sq = np.sqrt(den)
        res = c / sq / scale
        J = np.zeros((n, 5))
        for k in range(5):
            da, db = x0 @ dE[k].T, x1 @ dE[k]
            dc = np.sum(x1 * da, 1)
            dd = 2.0 * (((a[:, 0] * da[:, 0] + a[:, 1] * da[:, 1]) + b[:, 0] * db[:, 0]) + b[:, 1] * db[:, 1])
            J[:, k] = (dc / sq - 0.5 * c * dd / (den * sq)) / scale
        s = res * res
        ok = np.isfinite(s) & np.isfinite(J).all(1)
        w = np.where(ok, 1.0 / (1.0 + s), 0.0)
        J, res = np.where(ok[:, None], J, 0.0), np.where(ok, res, 0.0)
        cost = float(np.sum(np.where(ok, np.log1p(np.where(ok, s, 0.0)), 0.0)))
        H = np.einsum("n,ni,nj->ij", w, J, J)
        g = np.einsum("n,ni,n->i", w, J, res)
    return cost, H, g


def _solve5(H, g, lam):
    H6, g6 = np.eye(6), np.zeros(6)      # the 6 x 6 Cholesky of the pose stage, the sixth unknown pinned
    H6[:5, :5], g6[:5] = H, g
    d = PR.chol_solve6(H6, g6, lam)
    return None if d is None else d[:5]


def update(R, t, d):
    b1, b2 = tangent_basis(t)
    t1 = (t + d[3] * b1) + d[4] * b2
    return PR.rodrigues(d[:3]) @ R, t1 / np.sqrt(t1 @ t1)


def refine(rows, mask, R, t, scale: float, iters: int):
    R, t = R.copy(), t.copy()
    lam = LM_LAMBDA0
    cost, H, g = lm_pass(rows, mask, R, t, scale)
    for _ in range(iters):
        d = _solve5(H, g, lam)
        if d is None:
            lam *= 10.0
            continue
        R1, t1 = update(R, t, d)
        c1, H1, g1 = lm_pass(rows, mask, R1, t1, scale)
        if c1 < cost:
            R, t, cost, H, g = R1, t1, c1, H1, g1
            lam = max(lam * 0.1, 1e-15)
        else:
            lam *= 10.0
    return R, t


def inlier_mask(E9, rows, thr2: float):
    with np.errstate(**_IGN):
        return sampson(np.asarray(E9).reshape(1, 9), rows)[0] <= thr2


# ---------------------------------------------------------------- one pair, all stages
def estimate_pair(rows, f0: float, f1: float, p: int = 0, **params) -> dict:
    """rows: :func:`pair_rows`; f0, f1: the mean focal lengths of the two cameras; p: the pair's position among the processed pairs."""
    q = {**DEFAULTS, **params}
    n = rows.shape[0]
    fail = {"success": False, "E": np.zeros(9), "qvec": np.zeros(4), "tvec": np.zeros(3), "keep": np.zeros(n, dtype=bool), "num_inliers": 0,
            "num_front": 0, "best": -1, "n0": 0}
    if n < 5:
        return fail
    thr2 = threshold2(q["max_error"], f0, f1)
    scale = 1.0 * 0.5 * (1.0 / f0 + 1.0 / f1)
    E, n_sol, _ = hypotheses(rows, q["seed"], p, q["trials"])
    cnt, res = score(E, n_sol, rows, thr2)
    best = PR.rank(cnt, res, cnt >= 0)
    if best < 0:
        return fail
    n0 = int(cnt[best])
    fail["best"], fail["n0"] = best, n0
    Eh = E.reshape(-1, 9)[best]
    m0 = inlier_mask(Eh, rows, thr2)
    cands = decompose(Eh)
    fronts = [int((front_mask(R, t, rows) & m0).sum()) for R, t in cands]
    R0, t0 = cands[int(np.argmax(fronts))]
    ok0 = np.isfinite(R0).all() and np.isfinite(t0).all()
    R2, t2, m2, E2, refined = R0, t0, m0, Eh, False
    if ok0:
        R1, t1 = refine(rows, m0, R0, t0, scale, q["refine_iters"])
        m1 = inlier_mask(essential_of(R1, t1), rows, thr2)
        Rr, tr = refine(rows, m1, R1, t1, scale, q["refine_iters"])
        Er = essential_of(Rr, tr)
        mr = inlier_mask(Er, rows, thr2)
        if int(mr.sum()) >= n0 and np.isfinite(Rr).all() and np.isfinite(tr).all():
            R2, t2, m2, E2, refined = Rr, tr, mr, Er, True
    support = int(m2.sum())
    if not ok0 or support < max(q["min_num_inliers"], q["min_inlier_ratio"] * n):
        return fail
    return {"success": True, "refined": refined, "E": E2, "qvec": PR.rot_to_qvec(R2), "tvec": t2, "R": R2, "keep": m2, "num_inliers": support,
            "num_front": int((front_mask(R2, t2, rows) & m2).sum()), "best": best, "n0": n0, "E_hyp": Eh, "thr2": thr2}


# ---------------------------------------------------------------- planted scenes
def make_scene(seed: int, cam0, cam1, n: int, outlier_share: float, planar: bool = False, noise_px: float = 0.5, rotation_only: bool = False) -> dict:
    """Two cameras (frame 0 at the origin, frame 1 = R x + t), n points seen by both (a plane for ``planar``), uniform pixel noise
    within noise_px, and a share of matches whose frame-1 keypoint is replaced by a uniform one.  Keypoints are float32 pixels
    without the + 0.5.  -> dict(frames, cameras, matches [n, 2] shuffled indices, R, t (unit), outlier [n])."""
    rng = np.random.default_rng(seed)
    (m0, p0), (m1, p1) = PR.camera_row(cam0), PR.camera_row(cam1)
    w0, h0 = cam0[1], cam0[2]
    fx, fy, cx, cy = PR.unify(m0, p0)[:4]
    R = PR.rodrigues(rng.uniform(-0.25, 0.25, 3))
    t = np.zeros(3) if rotation_only else rng.uniform(-1.0, 1.0, 3) * np.array([1.0, 0.6, 0.4])
    X = np.zeros((0, 3))
    while X.shape[0] < n:      # points inside both images
        u, v = rng.uniform(0.05 * w0, 0.95 * w0, 4 * n), rng.uniform(0.05 * h0, 0.95 * h0, 4 * n)
        xn, yn = (u - cx) / fx, (v - cy) / fy
        z = 6.0 / (1.0 + 0.3 * xn - 0.2 * yn) if planar else rng.uniform(3.0, 12.0, 4 * n)
        P = np.stack([xn * z, yn * z, z], 1)
        px1, z1 = PR.project(P, R, t, m1, p1)
        ok = (z1 > 0.5) & (px1[:, 0] > 0.05 * cam1[1]) & (px1[:, 0] < 0.95 * cam1[1]) & (px1[:, 1] > 0.05 * cam1[2]) & (px1[:, 1] < 0.95 * cam1[2])
        X = np.concatenate([X, P[ok]])
    X = X[:n]
    px0, _ = PR.project(X, np.eye(3), np.zeros(3), m0, p0)
    px1, _ = PR.project(X, R, t, m1, p1)
    px0 = px0 + rng.uniform(-noise_px, noise_px, (n, 2))
    px1 = px1 + rng.uniform(-noise_px, noise_px, (n, 2))
    n_out = int(round(outlier_share * n))
    out_rows = rng.permutation(n)[:n_out]
    px1[out_rows] = np.stack([rng.uniform(0, cam1[1], n_out), rng.uniform(0, cam1[2], n_out)], 1)
    is_out = np.zeros(n, dtype=bool)
    is_out[out_rows] = True
    perm = rng.permutation(n)      # frame 1 stores its keypoints in another order
    kp1 = np.zeros((n, 2))
    kp1[perm] = px1
    nt = np.linalg.norm(t)
    return {"frames": [{"keypoints": (px0 - 0.5).astype(np.float32)}, {"keypoints": (kp1 - 0.5).astype(np.float32)}], "cameras": [cam0, cam1],
            "matches": np.stack([np.arange(n), perm], 1), "R": R, "t": t / nt if nt > 0 else t, "outlier": is_out, "n": n, "planar": planar}


def scene_rows(s: dict):
    """-> (rows [n, 4], f0, f1) of a scene's one pair, through the restatement's own normalisation (keypoint + 0.5)"""
    out = []
    for f, cam in zip(s["frames"], s["cameras"]):
        m, p = PR.camera_row(cam)
        out.append((PR.prepare(f["keypoints"], m, p), PR.f_mean(m, p)))
    norm = np.concatenate([out[0][0], out[1][0]])
    off = np.array([0, s["n"], 2 * s["n"]])
    return pair_rows(norm, off, 0, 1, s["matches"]), out[0][1], out[1][1]


SCENES = (      # (count, outlier share, planar): the counts of the end-to-end test; 65 and 257 sit one past a wave and a workgroup
    (40, 0.3, False), (64, 0.5, True), (65, 0.3, False), (257, 0.5, False), (1000, 0.3, True), (2048, 0.5, False), (150, 0.5, False), (300, 0.3, True))


def scenes(seed: int = 300) -> list:
    cams = list(PR.SCENE_CAMERAS.values())
    return [make_scene(seed + i, cams[i % 5], cams[(i + 2) % 5], n, share, planar) for i, (n, share, planar) in enumerate(SCENES)]


def pose_errors(R, t, s: dict):
    """(rotation error, angle between translation directions), degrees"""
    c = np.clip((np.trace(R @ s["R"].T) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.degrees(np.arccos(np.clip(t @ s["t"], -1.0, 1.0))))


def scipy_refine(rows, mask, R, t, scale: float):
    """An independent minimiser of the same Cauchy-Sampson cost on the same inlier set: scipy.optimize.minimize (BFGS, numerical
    gradient) over the same 5 parameters, restarted until the cost stops falling."""
    from scipy.optimize import minimize
    r = rows[mask]
    n = r.shape[0]
    x0 = np.concatenate([r[:, 0:2], np.ones((n, 1))], 1)
    x1 = np.concatenate([r[:, 2:4], np.ones((n, 1))], 1)

    def cost(d, R0, t0):
        R1, t1 = update(R0, t0, d * 1e-3)
        E = _skew(t1) @ R1
        a, b = x0 @ E.T, x1 @ E
        c = np.sum(x1 * a, 1)
        den = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
        return float(np.sum(np.log1p(c * c / den / (scale * scale))))

    last = np.inf
    for _ in range(6):
        sol = minimize(cost, np.zeros(5), args=(R, t), method="BFGS", options={"gtol": 1e-10, "maxiter": 500})
        R, t = update(R, t, sol.x * 1e-3)
        if not sol.fun < last - 1e-12 * abs(last):
            break
        last = sol.fun
    return R, t


def batch(scene_list):
    """Scenes -> (frames, cameras, pairs, matches) of one call: scene i is frames 2 i and 2 i + 1 and pair i."""
    frames = [f for s in scene_list for f in s["frames"]]
    cameras = [c for s in scene_list for c in s["cameras"]]
    return frames, cameras, np.array([(2 * i, 2 * i + 1) for i in range(len(scene_list))]).reshape(-1, 2), [s["matches"] for s in scene_list]
