"""Numpy float64 restatement of the bundle adjustment (csrc/bundle.hip) for the tests of
pram_amd.localization.bundle, in the kernels' order of operations: the linearisation of every observation (the residual and the
point Jacobian are tests/triangulation_ref.py's Track, the observation model the kernels share), the point and frame blocks, the
conjugate gradients on the reduced camera system, the Levenberg-Marquardt loop with its decisions and the final filter.  Sums run
as on the device: per point by :func:`TR.wave_sum`, per frame by :func:`frame_sum` (256 threads, the butterfly per wave, the fixed
4-wave fold), over frames by :func:`blocked_sum`.  The library is built without contraction, so the two differ by the rounding of
the transcendental functions only.  :func:`run` also returns the margins of every discrete decision.  :func:`dense_run` is an
independent form: the full normal equations over all poses and points, solved with numpy.linalg.solve.  Also the scenes the CPU
and GPU tests share."""
from __future__ import annotations

import numpy as np

from tests import pose_ref as PR
from tests import triangulation_ref as TR

BLOCK = 64            # PRAM_BA_BLOCK
OBS_DOUBLES = 20      # PRAM_BA_OBS_DOUBLES
DEFAULTS = dict(max_iters=40, cg_iters=60, cg_tol=1e-2, ftol=1e-6, loss_scale=1.0, lam0=PR.LM_LAMBDA0, max_reproj_error=4.0, min_tri_angle=1.5)
_IGN = dict(all="ignore")


# ---------------------------------------------------------------- the fixed orders
def frame_sum(v):
    """Sum over the leading axis as a workgroup of 256 does: thread t adds entries t, t + 256, ... in ascending order, every wave
    runs the xor butterfly, the four waves fold as ((w0 + w1) + w2) + w3."""
    v = np.asarray(v, dtype=np.float64)
    part = np.zeros((256,) + v.shape[1:])
    for k in range(v.shape[0]):
        part[k % 256] = part[k % 256] + v[k]
    lanes = np.arange(64)
    w = []
    for i in range(4):
        q = part[i * 64:(i + 1) * 64]
        for o in (32, 16, 8, 4, 2, 1):
            q = q + q[lanes ^ o]
        w.append(q[0])
    return ((w[0] + w[1]) + w[2]) + w[3]


def blocked_sum(v) -> float:
    """Blocks of BLOCK consecutive values added to 0.0 in ascending order, the block partials added to 0.0 in ascending order."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    total = 0.0
    for a in range(0, v.shape[0], BLOCK):
        s = 0.0
        for x in v[a:a + BLOCK].tolist():
            s = s + x
        total = total + s
    return float(total)


def _dot6(a, b):
    """Per frame: sum over the six parameters in ascending order, added to 0.0."""
    s = np.zeros(a.shape[0])
    for k in range(6):
        s = s + a[:, k] * b[:, k]
    return s


# ---------------------------------------------------------------- the problem
class Problem:
    """The tables of pram_ba_begin on the host, and the state (table, xyz)."""

    def __init__(self, keypoints, cam_model, cam_params, table, xyz, tabs: dict, frozen):
        self.kp = np.asarray(keypoints, dtype=np.float32)
        self.cam_model, self.cam_params = np.asarray(cam_model), np.asarray(cam_params, dtype=np.float64)
        self.table, self.xyz = np.array(table, dtype=np.float64), np.array(xyz, dtype=np.float64).reshape(-1, 3)
        for k in ("obs_row", "obs_frame", "obs_point", "frm_off", "pt_off", "pt_obs"):
            setattr(self, k, np.asarray(tabs[k], dtype=np.int64))
        self.F, self.P, self.O = self.table.shape[0], self.xyz.shape[0], self.obs_row.shape[0]
        cnt = np.diff(self.frm_off)
        self.fmask = np.where(cnt > 0, np.asarray(frozen, dtype=np.int64) & 63, 63)
        scene = {"table": self.table, "cam_model": self.cam_model, "cam_params": self.cam_params, "keypoints": self.kp,
                 "norm05": np.zeros((self.kp.shape[0], 2))}
        self.track = TR.Track(scene, self.obs_row, self.obs_frame)      # cameras and keypoints + 0.5 per observation

    def residual(self, table, xyz, with_jac: bool = False):
        self.track.T = table[self.obs_frame]
        return self.track.residual(xyz[self.obs_point].T, with_jac=with_jac)


def linearise(pr: Problem, table, xyz, loss_scale: float = 1.0):
    """-> J [O, 20] (sqrt(w) J_c [2][6], sqrt(w) J_p [2][3], sqrt(w) r [2]), ok [O], and the unweighted pieces for the tests."""
    z, r0, r1, Jp = pr.residual(table, xyz, with_jac=True)
    T, X = table[pr.obs_frame], xyz[pr.obs_point]
    with np.errstate(**_IGN):
        s = (r0 * r0 + r1 * r1) / (loss_scale * loss_scale)
        ok = (z > 1e-12) & np.isfinite(s)
        sw = np.sqrt(1.0 / (1.0 + s))
        Y0 = T[:, 0] * X[:, 0] + T[:, 1] * X[:, 1] + T[:, 2] * X[:, 2]
        Y1 = T[:, 3] * X[:, 0] + T[:, 4] * X[:, 1] + T[:, 5] * X[:, 2]
        Y2 = T[:, 6] * X[:, 0] + T[:, 7] * X[:, 1] + T[:, 8] * X[:, 2]
        J = np.zeros((pr.O, OBS_DOUBLES))
        Jc = np.zeros((pr.O, 2, 6))
        for i in range(2):
            jp = Jp[:, i * 3:i * 3 + 3]
            a0 = jp[:, 0] * T[:, 0] + jp[:, 1] * T[:, 1] + jp[:, 2] * T[:, 2]
            a1 = jp[:, 0] * T[:, 3] + jp[:, 1] * T[:, 4] + jp[:, 2] * T[:, 5]
            a2 = jp[:, 0] * T[:, 6] + jp[:, 1] * T[:, 7] + jp[:, 2] * T[:, 8]
            jc = np.stack([a2 * Y1 - a1 * Y2, a0 * Y2 - a2 * Y0, a1 * Y0 - a0 * Y1, a0, a1, a2], 1)
            Jc[:, i] = jc
            frozen = ((pr.fmask[pr.obs_frame][:, None] >> np.arange(6)[None]) & 1).astype(bool)
            J[:, i * 6:i * 6 + 6] = np.where(frozen, 0.0, sw[:, None] * jc)
            J[:, 12 + i * 3:15 + i * 3] = sw[:, None] * jp
        J[:, 18], J[:, 19] = sw * r0, sw * r1
    J[~ok] = 0.0
    return J, ok, {"z": z, "r": np.stack([r0, r1], 1), "s": s, "Jc": Jc, "Jp": Jp.reshape(-1, 2, 3)}


def _vinv_mul(V, a):
    return np.stack([V[..., 0] * a[..., 0] + V[..., 1] * a[..., 1] + V[..., 2] * a[..., 2],
                     V[..., 1] * a[..., 0] + V[..., 3] * a[..., 1] + V[..., 4] * a[..., 2],
                     V[..., 2] * a[..., 0] + V[..., 4] * a[..., 1] + V[..., 5] * a[..., 2]], -1)


def point_blocks(pr: Problem, J, ok, lam: float):
    """-> Vinv [P, 6] (zeros for a point that cannot move), g_p [P, 3], solvable [P]."""
    Vinv, gp, good = np.zeros((pr.P, 6)), np.zeros((pr.P, 3)), np.zeros(pr.P, dtype=bool)
    for p in range(pr.P):
        o = pr.pt_obs[pr.pt_off[p]:pr.pt_off[p + 1]]
        j, r0, r1 = J[o, 12:18], J[o, 18], J[o, 19]
        terms = np.stack([j[:, 0] * j[:, 0] + j[:, 3] * j[:, 3], j[:, 0] * j[:, 1] + j[:, 3] * j[:, 4], j[:, 0] * j[:, 2] + j[:, 3] * j[:, 5],
                          j[:, 1] * j[:, 1] + j[:, 4] * j[:, 4], j[:, 1] * j[:, 2] + j[:, 4] * j[:, 5], j[:, 2] * j[:, 2] + j[:, 5] * j[:, 5],
                          j[:, 0] * r0 + j[:, 3] * r1, j[:, 1] * r0 + j[:, 4] * r1, j[:, 2] * r0 + j[:, 5] * r1], 1)
        acc = TR.wave_sum(terms) if len(o) else np.zeros(9)
        gp[p] = acc[6:]
        A = np.array([acc[0] + lam * acc[0], acc[1], acc[2], acc[3] + lam * acc[3], acc[4], acc[5] + lam * acc[5]])
        cols = [TR.chol_solve3(A, e) for e in np.eye(3)] if int(ok[o].sum()) >= 2 else [None]
        if all(c is not None for c in cols):
            Vinv[p] = [cols[0][0], cols[0][1], cols[0][2], cols[1][1], cols[1][2], cols[2][2]]
            good[p] = True
    return Vinv, gp, good


def _w_terms(j):
    """Per observation W = J_c^T J_p [6][3]."""
    return np.stack([np.stack([j[:, a] * j[:, 12 + k] + j[:, 6 + a] * j[:, 15 + k] for k in range(3)], 1) for a in range(6)], 1)


def frame_blocks(pr: Problem, J, Vinv, gp, lam: float):
    """-> S's diagonal blocks [F, 21] (damped; a frozen parameter's diagonal 1), diag U [F, 6], b [F, 6]."""
    S, dU, b = np.zeros((pr.F, 21)), np.zeros((pr.F, 6)), np.zeros((pr.F, 6))
    for f in range(pr.F):
        a0, a1 = pr.frm_off[f], pr.frm_off[f + 1]
        j, p = J[a0:a1], pr.obs_point[a0:a1]
        W = _w_terms(j)
        WV = np.stack([_vinv_mul(Vinv[p], W[:, a]) for a in range(6)], 1)
        cols = []
        for a in range(6):
            for c in range(a, 6):
                u = j[:, a] * j[:, c] + j[:, 6 + a] * j[:, 6 + c]
                w = WV[:, a, 0] * W[:, c, 0] + WV[:, a, 1] * W[:, c, 1] + WV[:, a, 2] * W[:, c, 2]
                cols.append(u - w)
        cols += [j[:, a] * j[:, a] + j[:, 6 + a] * j[:, 6 + a] for a in range(6)]
        cols += [j[:, a] * j[:, 18] + j[:, 6 + a] * j[:, 19] for a in range(6)]
        cols += [WV[:, a, 0] * gp[p, 0] + WV[:, a, 1] * gp[p, 1] + WV[:, a, 2] * gp[p, 2] for a in range(6)]
        tot = frame_sum(np.stack(cols, 1)) if a1 > a0 else np.zeros(39)
        e = 0
        for a in range(6):
            for c in range(a, 6):
                v = tot[e]
                if a == c:
                    v = 1.0 if (pr.fmask[f] >> a) & 1 else v + lam * tot[21 + a]
                S[f, e] = v
                e += 1
        dU[f], b[f] = tot[21:27], tot[33:39] - tot[27:33]
    return S, dU, b


def _sym6(Su):
    M = np.zeros((6, 6))
    e = 0
    for a in range(6):
        for c in range(a, 6):
            M[a, c] = M[c, a] = Su[e]
            e += 1
    return M


def precond(S, r):
    """Per frame M z = r by chol_solve6's factorisation; a block that does not factor leaves z = r."""
    z = np.zeros_like(r)
    for f in range(r.shape[0]):
        x = PR.chol_solve6(_sym6(S[f]), -r[f], 0.0)
        z[f] = r[f] if x is None else x
    return z


def mv_points(pr: Problem, J, Vinv, v):
    """Per point: V^-1 sum J_p^T J_c v_c -> (y [P, 3], the sums before V^-1)."""
    vf = v[pr.obs_frame]
    t0, t1 = np.zeros(pr.O), np.zeros(pr.O)
    for a in range(6):
        t0 = t0 + J[:, a] * vf[:, a]
        t1 = t1 + J[:, 6 + a] * vf[:, a]
    terms = np.stack([J[:, 12 + c] * t0 + J[:, 15 + c] * t1 for c in range(3)], 1)
    acc = np.zeros((pr.P, 3))
    for p in range(pr.P):
        o = pr.pt_obs[pr.pt_off[p]:pr.pt_off[p + 1]]
        if len(o):
            acc[p] = TR.wave_sum(terms[o])
    return _vinv_mul(Vinv, acc), acc


def matvec(pr: Problem, J, Vinv, dU, lam: float, v):
    """q = S v: the two passes of the device."""
    y, _ = mv_points(pr, J, Vinv, v)
    vf, yo = v[pr.obs_frame], y[pr.obs_point]
    t0, t1 = np.zeros(pr.O), np.zeros(pr.O)
    for a in range(6):
        t0 = t0 + J[:, a] * vf[:, a]
        t1 = t1 + J[:, 6 + a] * vf[:, a]
    t0 = t0 - (J[:, 12] * yo[:, 0] + J[:, 13] * yo[:, 1] + J[:, 14] * yo[:, 2])
    t1 = t1 - (J[:, 15] * yo[:, 0] + J[:, 16] * yo[:, 1] + J[:, 17] * yo[:, 2])
    terms = np.stack([J[:, a] * t0 + J[:, 6 + a] * t1 for a in range(6)], 1)
    q = np.zeros((pr.F, 6))
    for f in range(pr.F):
        a0, a1 = pr.frm_off[f], pr.frm_off[f + 1]
        tot = frame_sum(terms[a0:a1]) if a1 > a0 else np.zeros(6)
        frozen = ((pr.fmask[f] >> np.arange(6)) & 1).astype(bool)
        q[f] = np.where(frozen, v[f], tot + lam * dU[f] * v[f])
    return q


def pcg(pr: Problem, J, Vinv, S, dU, b, lam: float, cg_iters: int, cg_tol: float):
    """-> (x [F, 6], iterations, trace): trace["stop"] holds, per iteration, |r| / (cg_tol |b|)."""
    x, r = np.zeros_like(b), b.copy()
    z = precond(S, r)
    p = z.copy()
    rz, bb = blocked_sum(_dot6(r, z)), blocked_sum(_dot6(r, r))
    tr = {"stop": [], "fail": 0, "first": {"z": z.copy(), "rz": rz, "bb": bb}}
    it = 0
    if not bb > 0.0:
        return x, it, tr
    for _ in range(cg_iters):
        q = matvec(pr, J, Vinv, dU, lam, p)
        pap = blocked_sum(_dot6(p, q))
        if it == 0:
            tr["first"].update(q=q.copy(), pap=pap)
        with np.errstate(**_IGN):
            alpha = rz / pap
        if not pap > 0.0 or not np.isfinite(alpha):
            tr["fail"] += 1
            break
        x = x + alpha * p
        r = r - alpha * q
        z = precond(S, r)
        rz_new, rr = blocked_sum(_dot6(r, z)), blocked_sum(_dot6(r, r))
        with np.errstate(**_IGN):
            beta = rz_new / rz
        rz = rz_new
        it += 1
        tr["stop"].append(float(np.sqrt(rr) / (cg_tol * np.sqrt(bb))))
        if np.sqrt(rr) <= cg_tol * np.sqrt(bb) or not np.isfinite(beta):
            break
        p = z + beta * p
    return x, it, tr


def rodrigues_update(T, d):
    """pose_update of ransac.h on a row of the frame table, with the centre recomputed as pram_tri_frames does."""
    if not np.any(d != 0.0):
        return T.copy()
    R, t = T[:9].reshape(3, 3), T[9:12]
    th = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if th < 1e-12:
        E = np.array([[1.0, -d[2], d[1]], [d[2], 1.0, -d[0]], [-d[1], d[0], 1.0]])
    else:
        kx, ky, kz = d[0] / th, d[1] / th, d[2] / th
        K = np.array([[0.0, -kz, ky], [kz, 0.0, -kx], [-ky, kx, 0.0]])
        sn, cs = np.sin(th), 1.0 - np.cos(th)
        E = np.zeros((3, 3))
        for a in range(3):
            for c in range(3):
                kk = K[a, 0] * K[0, c] + K[a, 1] * K[1, c] + K[a, 2] * K[2, c]
                E[a, c] = (1.0 if a == c else 0.0) + sn * K[a, c] + cs * kk
    out = T.copy()
    Rn = np.array([[E[a, 0] * R[0, c] + E[a, 1] * R[1, c] + E[a, 2] * R[2, c] for c in range(3)] for a in range(3)])
    tn = t + d[3:]
    out[:9], out[9:12] = Rn.reshape(-1), tn
    for k in range(3):
        out[12 + k] = -(Rn[0, k] * tn[0] + Rn[1, k] * tn[1] + Rn[2, k] * tn[2])
    return out


def cost(pr: Problem, table, xyz, loss_scale: float = 1.0) -> float:
    z, r0, r1 = pr.residual(table, xyz)
    with np.errstate(**_IGN):
        s = (r0 * r0 + r1 * r1) / (loss_scale * loss_scale)
        ok = (z > 1e-12) & np.isfinite(s)
        terms = np.where(ok, np.log1p(np.where(ok, s, 0.0)), 0.0)
    per_frame = [float(frame_sum(terms[a:b])) if b > a else 0.0 for a, b in zip(pr.frm_off[:-1], pr.frm_off[1:])]
    return blocked_sum(per_frame)


def lm_step(pr: Problem, table, xyz, J, ok, lam: float, p: dict):
    """One iteration up to the candidate -> (table_c, xyz_c, d_c, cg iterations, traces, solvable points)."""
    Vinv, gp, good = point_blocks(pr, J, ok, lam)
    S, dU, b = frame_blocks(pr, J, Vinv, gp, lam)
    x, n_cg, tr = pcg(pr, J, Vinv, S, dU, b, lam, p["cg_iters"], p["cg_tol"])
    _, acc = mv_points(pr, J, Vinv, x)
    xyz_c = xyz - _vinv_mul(Vinv, gp + acc)
    table_c = np.stack([rodrigues_update(table[f], x[f]) for f in range(pr.F)])
    tr.update(Vinv=Vinv, gp=gp, S=S, dU=dU, b=b)
    return table_c, xyz_c, x, n_cg, tr, good


def filter_points(pr: Problem, table, xyz, max_reproj_error: float, min_tri_angle: float, loss_scale: float = 1.0) -> dict:
    z, r0, r1 = pr.residual(table, xyz)
    with np.errstate(**_IGN):
        e2 = r0 * r0 + r1 * r1
        keep = (z > 0.0) & (e2 <= max_reproj_error * max_reproj_error)
        err = np.sqrt(e2)
        zero_w = ~((z > 1e-12) & np.isfinite(e2 / (loss_scale * loss_scale)))
    min_angle = float(np.deg2rad(min_tri_angle))
    C = table[:, 12:15]
    pt_keep, pt_err, pt_ang, pt_cnt = np.zeros(pr.P, dtype=bool), np.zeros(pr.P), np.full(pr.P, -1.0), np.zeros(pr.P, dtype=np.int64)
    for p in range(pr.P):
        o = pr.pt_obs[pr.pt_off[p]:pr.pt_off[p + 1]]
        k = o[keep[o]]
        pt_cnt[p] = len(k)
        kept_err = np.where(keep[o], err[o], 0.0)
        pt_err[p] = float(TR.wave_sum(kept_err)) / len(k) if len(k) else 0.0
        rays = [xyz[p] - C[pr.obs_frame[i]] for i in k.tolist()]
        angles = [TR.angle(rays[a], rays[c]) for a in range(len(rays)) for c in range(a + 1, len(rays))]
        pt_ang[p] = max(angles) if angles else -1.0
        pt_keep[p] = len(k) >= 2 and pt_ang[p] >= min_angle
    return {"obs_keep": keep, "obs_error": err, "pt_keep": pt_keep, "pt_error": pt_err, "pt_angle": pt_ang, "pt_kept": pt_cnt,
            "zero_weight": int(zero_w.sum()), "filtered_observations": int((~keep).sum())}


def run(pr: Problem, **params) -> dict:
    """The whole adjustment -> table, xyz, the report's numbers, the filter, and ``margins``: per LM iteration the relative
    distance of the accept test from equality and of every CG stop test from its threshold."""
    p = {**DEFAULTS, **params}
    table, xyz, lam = pr.table.copy(), pr.xyz.copy(), float(p["lam0"])
    c0 = c = cost(pr, table, xyz, p["loss_scale"])
    accepted, cg_counts, accept_margin, cg_margin, fails = [], [], [], [], 0
    reason, good, first = "max_iters", np.ones(pr.P, dtype=bool), None
    J = ok = None
    moved = np.zeros(pr.F, dtype=bool)
    for it in range(p["max_iters"]):
        if J is None:
            J, ok, _ = linearise(pr, table, xyz, p["loss_scale"])
        table_c, xyz_c, x, n_cg, tr, good = lm_step(pr, table, xyz, J, ok, lam, p)
        if first is None:
            first = {"J": J.copy(), "ok": ok.copy(), "x": x.copy(), **tr}
        c1 = cost(pr, table_c, xyz_c, p["loss_scale"])
        acc = bool(c1 < c)
        accepted.append(acc); cg_counts.append(n_cg); fails += tr["fail"]
        accept_margin.append(abs(c1 - c) / c if np.isfinite(c1) and c > 0 else np.inf)
        cg_margin.append(min([abs(s - 1.0) for s in tr["stop"]], default=np.inf))
        if acc:
            rel = (c - c1) / c
            table, xyz, c = table_c, xyz_c, c1
            moved |= np.any(x != 0.0, axis=1)
            lam = max(lam * 0.1, 1e-15)
            J = None
            if rel < p["ftol"]:
                reason = "ftol"
                break
        else:
            lam = lam * 10.0
    flt = filter_points(pr, table, xyz, p["max_reproj_error"], p["min_tri_angle"], p["loss_scale"])
    return {"table": table, "xyz": xyz, "initial_cost": c0, "final_cost": c, "accepted": np.array(accepted, dtype=bool),
            "cg_iterations": np.array(cg_counts, dtype=np.int64), "lam": lam, "termination": reason, "moved": moved, "solvable": good,
            "cg_breakdowns": fails, "first": first, "filter": flt,
            "margins": {"accept": np.array(accept_margin), "cg": np.array(cg_margin)}}


# ---------------------------------------------------------------- the independent dense form
def dense_jacobian(pr: Problem, table, xyz, loss_scale: float = 1.0):
    """-> (Jd [2 O, 6 F + 3 P], rd [2 O]) of the weighted problem, frozen columns zero."""
    J, ok, _ = linearise(pr, table, xyz, loss_scale)
    Jd, rd = np.zeros((2 * pr.O, 6 * pr.F + 3 * pr.P)), np.zeros(2 * pr.O)
    for o in range(pr.O):
        f, p = pr.obs_frame[o], pr.obs_point[o]
        for i in range(2):
            Jd[2 * o + i, 6 * f:6 * f + 6] = J[o, i * 6:i * 6 + 6]
            Jd[2 * o + i, 6 * pr.F + 3 * p:6 * pr.F + 3 * p + 3] = J[o, 12 + i * 3:15 + i * 3]
            rd[2 * o + i] = J[o, 18 + i]
    weighted = np.bincount(pr.obs_point[ok], minlength=pr.P)
    for p in np.nonzero(weighted < 2)[0].tolist():      # a point with fewer than two weighted observations stays
        Jd[:, 6 * pr.F + 3 * p:6 * pr.F + 3 * p + 3] = 0.0
    return Jd, rd


def dense_step(pr: Problem, table, xyz, lam: float, loss_scale: float = 1.0):
    """(H + lam diag H) d = -g over every parameter at once; a parameter whose column is zero gets a unit diagonal."""
    Jd, rd = dense_jacobian(pr, table, xyz, loss_scale)
    H, g = Jd.T @ Jd, Jd.T @ rd
    dg = np.diag(H).copy()
    H = H + lam * np.diag(dg)
    dead = dg == 0.0
    H[dead, dead] = 1.0
    return np.linalg.solve(H, -g), H, g


def dense_run(pr: Problem, **params) -> dict:
    """Levenberg-Marquardt with the device's accept rule on the dense normal equations (no Schur complement, no CG)."""
    p = {**DEFAULTS, **params}
    table, xyz, lam = pr.table.copy(), pr.xyz.copy(), float(p["lam0"])
    c = c0 = cost(pr, table, xyz, p["loss_scale"])
    n = 0
    for _ in range(p["max_iters"]):
        d, _, _ = dense_step(pr, table, xyz, lam, p["loss_scale"])
        table_c = np.stack([rodrigues_update(table[f], d[6 * f:6 * f + 6]) for f in range(pr.F)])
        xyz_c = xyz + d[6 * pr.F:].reshape(-1, 3)
        c1 = cost(pr, table_c, xyz_c, p["loss_scale"])
        n += 1
        if c1 < c:
            rel = (c - c1) / c
            table, xyz, c, lam = table_c, xyz_c, c1, max(lam * 0.1, 1e-15)
            if rel < p["ftol"]:
                break
        else:
            lam *= 10.0
    return {"table": table, "xyz": xyz, "initial_cost": c0, "final_cost": c, "iterations": n}


def reduced_dense(pr: Problem, J, Vinv, dU, lam: float) -> np.ndarray:
    """The reduced camera matrix S [6 F, 6 F] written out from the blocks, for the matvec test."""
    Ud, Wd = np.zeros((6 * pr.F, 6 * pr.F)), np.zeros((6 * pr.F, 3 * pr.P))
    W = _w_terms(J)
    for o in range(pr.O):
        f, p = pr.obs_frame[o], pr.obs_point[o]
        jc = J[o, :12].reshape(2, 6)
        Ud[6 * f:6 * f + 6, 6 * f:6 * f + 6] += jc.T @ jc
        Wd[6 * f:6 * f + 6, 3 * p:3 * p + 3] += W[o]
    Ud = Ud + lam * np.diag(np.diag(Ud))
    Vd = np.zeros((3 * pr.P, 3 * pr.P))
    for p in range(pr.P):
        v = Vinv[p]
        Vd[3 * p:3 * p + 3, 3 * p:3 * p + 3] = [[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]]
    S = Ud - Wd @ Vd @ Wd.T
    for f in range(pr.F):
        for a in range(6):
            if (pr.fmask[f] >> a) & 1:
                S[6 * f + a, 6 * f + a] = 1.0
    return S


# ---------------------------------------------------------------- poses, errors, scenes
def table_pose(T):
    return T[:9].reshape(3, 3), T[9:12]


def pose_errors(table, table_gt):
    """-> (rotation error in degrees [F], centre error [F])."""
    rot, cen = [], []
    for a, b in zip(table, table_gt):
        Ra, Rb = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
        D = Ra @ Rb.T
        sn = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
        rot.append(np.degrees(np.arctan2(sn, (np.trace(D) - 1.0) / 2.0)))      # exact for small angles, where arccos is not
        cen.append(np.linalg.norm(a[12:15] - b[12:15]))
    return np.array(rot), np.array(cen)


def perturb_poses(s: dict, rot_deg: float, centre: float, seed: int, keep=()) -> tuple:
    """The scene's poses with a random rotation of about rot_deg degrees and a shift of the centre of about ``centre`` -> (qvec,
    tvec); the frames of ``keep`` stay."""
    rng = np.random.RandomState(seed)
    q, t = s["qvec"].copy(), s["tvec"].copy()
    for f in range(s["n_frames"]):
        if f in keep:
            continue
        R = PR.qvec_to_rot(s["qvec"][f])
        C = -R.T @ s["tvec"][f]
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w) * np.deg2rad(rot_deg) * rng.uniform(0.5, 1.0)
        Rn = PR.rodrigues(w) @ R
        Cn = C + rng.normal(size=3) / np.sqrt(3.0) * centre
        q[f], t[f] = PR.rot_to_qvec(Rn), -Rn @ Cn
    return q, t


def with_poses(s: dict, qvec, tvec) -> dict:
    """A copy of a triangulation scene with other poses (the table follows)."""
    out = dict(s)
    out["qvec"], out["tvec"] = np.asarray(qvec, dtype=np.float64), np.asarray(tvec, dtype=np.float64)
    out["table"] = TR.frame_table(out["qvec"], out["tvec"], s["cam_model"], s["cam_params"])
    return out


def model_of(s: dict, **params) -> dict:
    """The restated stages 2-4 on a scene -> triangulate_map's dict (triangulation.map_tables, host code)."""
    from pram_amd.localization import triangulation as TG
    r = TR.run(s, **params)
    return TG.map_tables(np.arange(s["n_frames"]), s["frame_off"], r["tracks"], r["tri"])


def problem_of(s: dict, model: dict, frozen=None, gauge: str = "colmap") -> tuple:
    """-> (Problem, the tables) as bundle_adjust builds them for the scene's poses."""
    from pram_amd.localization import bundle as BA
    tabs = BA.observation_tables(model, np.arange(s["n_frames"]), s["frame_off"])
    mask = BA.gauge_mask(gauge, frozen, tabs["frm_off"])
    return Problem(s["keypoints"], s["cam_model"], s["cam_params"], s["table"], model["point3D_xyzs"], tabs, mask), tabs


def planted_model(s: dict, min_len: int = 2) -> dict:
    """A model straight from a scene's planted points (``where``: (frame, point) -> keypoint), triangulate_map's shape: the points
    seen min_len times at least, at their planted positions."""
    seen = {}
    for (f, p), k in sorted(s["where"].items()):
        seen.setdefault(p, []).append((f, k))
    ids, xyz, tracks = [], [], {}
    for p in sorted(seen):
        if len(seen[p]) >= min_len:
            ids.append(p + 1)
            xyz.append(s["xyz"][p])
            tracks[p + 1] = (np.array([f for f, _ in seen[p]], dtype=np.int64), np.array([k for _, k in seen[p]], dtype=np.int64))
    return {"point_ids": np.array(ids, dtype=np.int64), "point3D_xyzs": np.array(xyz, dtype=np.float64).reshape(-1, 3),
            "track_error": np.zeros(len(ids)), "tracks": tracks, "point3D_frame_ids": {p: t[0] for p, t in tracks.items()}}


def planted_tracks(s: dict, min_len: int = 2) -> dict:
    """The planted points' observations as a track table (tests/triangulation_ref.py's ``tracks`` shape), entries by ascending row."""
    seen = {}
    for (f, p), k in s["where"].items():
        seen.setdefault(p, []).append(int(s["frame_off"][f]) + k)
    rows = [np.sort(np.array(seen[p], dtype=np.int64)) for p in sorted(seen) if len(seen[p]) >= min_len]
    off = np.zeros(len(rows) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    row = np.concatenate(rows).astype(np.int32)
    frame = (np.searchsorted(np.asarray(s["frame_off"]), row, side="right") - 1).astype(np.int32)
    return {"trk_off": off, "trk_label": np.array([r[0] for r in rows], dtype=np.int32), "trk_row": row, "trk_frame": frame,
            "trk_kpt": (row - np.asarray(s["frame_off"])[frame]).astype(np.int32),
            "point": np.array([p for p in sorted(seen) if len(seen[p]) >= min_len], dtype=np.int64)}


def triangulated_model(s: dict, max_reproj_error: float = 4.0, min_len: int = 2) -> tuple:
    """The planted tracks triangulated by the restated stage 4 with the scene's (possibly perturbed) poses -> (triangulate_map's
    dict, the planted point of every model point)."""
    from pram_amd.localization import triangulation as TG
    trk = planted_tracks(s, min_len)
    tri = TR.triangulate(s, trk, trials=128, seed=0, min_tri_angle=1.5, max_reproj_error=max_reproj_error)
    return TG.map_tables(np.arange(s["n_frames"]), s["frame_off"], trk, tri), trk["point"][tri["accept"]]


_scenes: dict = {}


def frames_scene(counts=(0, 1, 63, 64, 65, 257), noise: float = 0.3, seed: int = 3) -> dict:
    """Frames on an arc that hold exactly ``counts`` observations: 257 points, frame f sees the first counts[f] of them (so every
    point is seen by the last frame, the first 65 by three frames at least, point 0 by five), plus one frame of 200 observations
    that gives the points beyond 65 a second view."""
    key = ("frames", tuple(counts), noise, seed)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.RandomState(seed)
    counts = list(counts) + [200]
    F = len(counts)
    ang = np.deg2rad(np.linspace(-40.0, 40.0, F))
    centres = [np.array([8.0 * np.sin(a), 0.5 * np.cos(2 * a), -8.0 * np.cos(a)]) for a in ang]
    s = TR._base([TR.CAMERAS[f % 5] for f in range(F)], centres, [np.zeros(3)] * F)
    n = max(counts)
    xyz = rng.uniform([-1.8, -1.2, -1.8], [1.8, 1.2, 1.8], size=(n, 3))
    kps, where = [[] for _ in range(F)], {}
    for f in range(F):
        px, z = TR.project(s, f, xyz)
        pts = range(counts[f]) if f < F - 1 else range(n - counts[f], n)
        for p in rng.permutation(list(pts)).tolist():
            assert z[p] > 0 and 0 <= px[p, 0] < TR.WIDTH and 0 <= px[p, 1] < TR.HEIGHT
            kps[f].append(tuple(px[p] - 0.5 + rng.uniform(-noise, noise, size=2)))
            where[(f, p)] = len(kps[f]) - 1
    s.update(pairs=np.zeros((0, 2), dtype=np.int64), matches=[], xyz=xyz, where=where, counts=tuple(counts), noise=noise)
    _scenes[key] = TR._finish(s, kps)
    return _scenes[key]


# ---------------------------------------------------------------- the runs the GPU test makes (tests/test_bundle_cpu.py asserts their margins)
def add_point(model: dict, xyz, frames, kpts) -> int:
    """A further point in a model (in place): the next id, the given position and track."""
    pid = int(model["point_ids"].max()) + 1 if len(model["point_ids"]) else 1
    model["point_ids"] = np.append(model["point_ids"], pid)
    model["point3D_xyzs"] = np.vstack([model["point3D_xyzs"], np.asarray(xyz, dtype=np.float64).reshape(1, 3)])
    model["track_error"] = np.append(model["track_error"], 0.0)
    model["tracks"][pid] = (np.asarray(frames, dtype=np.int64), np.asarray(kpts, dtype=np.int64))
    model["point3D_frame_ids"][pid] = model["tracks"][pid][0]
    model.pop("frames", None)
    return pid


def _special_case() -> dict:
    """tri_scene with perturbed poses and, added by hand: a point behind one of its cameras, a gross outlier in a long track, and
    the planted point whose rays all meet below min_tri_angle."""
    s = TR.tri_scene()
    q, t = perturb_poses(s, 0.5, 0.15, seed=2, keep=(0,))
    sp = with_poses(s, q, t)
    model, planted = triangulated_model(sp, max_reproj_error=40.0)
    used = {int(sp["frame_off"][f]) + k for (f, p), k in s["where"].items()}
    (f4, k4), (f10, k10) = s["special_rows"]["behind"]
    used |= {int(sp["frame_off"][f4]) + k4, int(sp["frame_off"][f10]) + k10}
    T4 = s["table"][f4]
    n4 = TR.normalize(s["keypoints"][int(s["frame_off"][f4]) + k4][None], [0, 1], s["cam_model"][f4:f4 + 1], s["cam_params"][f4:f4 + 1], 0.5)[0]
    ray = T4[:9].reshape(3, 3).T @ np.array([n4[0], n4[1], 1.0])
    behind = add_point(model, T4[12:15] - 2.0 * ray, [f4, f10], [k4, k10])
    # the gross outlier: a detection of nothing in frame 7, added to the longest track that frame 7 does not see
    lens = {p: len(tk[0]) for p, tk in model["tracks"].items() if 7 not in tk[0].tolist() and p != behind}
    host = max(sorted(lens), key=lambda p: lens[p])
    free = [k for k in range(int(sp["frame_off"][8] - sp["frame_off"][7])) if int(sp["frame_off"][7]) + k not in used]
    img, kpt = model["tracks"][host]
    model["tracks"][host] = (np.append(img, 7), np.append(kpt, free[0]))
    model["point3D_frame_ids"][host] = model["tracks"][host][0]
    far = s["special"]["far"]
    fr = sorted(f for (f, p) in s["where"] if p == far)
    low = add_point(model, s["xyz"][far], fr, [s["where"][(f, far)] for f in fr])
    frozen = np.zeros(s["n_frames"], dtype=np.int64)
    frozen[0], frozen[9] = 63, 1 << 3
    return {"scene": sp, "truth": s, "model": model, "frozen": frozen, "params": {}, "behind": behind, "outlier": (host, 7, free[0]), "low_angle": low}


def _ring_case() -> dict:
    s = TR.ring_scene(lengths=(2, 3, 17, 63, 64, 65) + (30,) * 40)
    q, t = perturb_poses(s, 0.3, 0.05, seed=4, keep=(0,))
    sp = with_poses(s, q, t)
    model = planted_model(s)
    frozen = np.zeros(s["n_frames"], dtype=np.int64)
    frozen[0], frozen[1], frozen[30:] = 63, 1 << 3, 63      # the frames that see three points or fewer stay
    return {"scene": sp, "truth": s, "model": model, "frozen": frozen, "params": {"max_iters": 12}}


def _frames_case() -> dict:
    s = frames_scene()
    F = s["n_frames"]
    q, t = perturb_poses(s, 0.3, 0.05, seed=6, keep=(F - 2, F - 1))
    sp = with_poses(s, q, t)
    frozen = np.zeros(F, dtype=np.int64)
    frozen[F - 2:] = 63
    return {"scene": sp, "truth": s, "model": planted_model(s), "frozen": frozen, "params": {"max_iters": 12}}


def _two_case() -> dict:
    s = TR.ring_scene(lengths=(2,) * 30, n_frames=2, seed=8)
    q, t = perturb_poses(s, 0.3, 0.05, seed=9, keep=(0,))
    sp = with_poses(s, q, t)
    # the two cameras face each other along z, so COLMAP's frozen t_x would leave the scale free: the translation stays instead
    return {"scene": sp, "truth": s, "model": planted_model(s), "frozen": np.array([63, 0b111000]), "params": {"max_iters": 12}}


def _derived(base: str, **over):
    def make():
        c = dict(gpu_case(base))
        c.update({k: v for k, v in over.items() if k != "params"})
        c["params"] = {**c["params"], **over.get("params", {})}
        return c
    return make


GPU_RUNS = {"special": _special_case, "ring": _ring_case, "frames": _frames_case, "two": _two_case,
            "frozen_all": _derived("special", frozen="all"), "zero": _derived("special", params={"max_iters": 0})}
_cases: dict = {}


def gpu_case(name: str) -> dict:
    """-> scene (the poses the adjustment starts from), truth, model, frozen, params, and ``problem`` / ``tables``."""
    if name not in _cases:
        c = GPU_RUNS[name]()
        if isinstance(c["frozen"], str):
            c["frozen"] = np.full(c["scene"]["n_frames"], 63, dtype=np.int64)
        c["problem"], c["tables"] = problem_of(c["scene"], c["model"], frozen=c["frozen"])
        _cases[name] = c
    return _cases[name]


_runs: dict = {}


def gpu_run(name: str) -> dict:
    """The restated adjustment of a case, computed once."""
    if name not in _runs:
        c = gpu_case(name)
        _runs[name] = run(c["problem"], **c["params"])
    return _runs[name]
