"""Numpy float64 restatement of the bundle adjustment with camera groups (csrc/bundle.hip's pram_bac_* entries)
for the tests of pram_amd.localization.bundle's refine flags.  It builds on tests/bundle_ref.py (read only): its Problem, its
linearisation of the poses and points, its point and frame blocks and its fixed orders; what is added is the second kind of
unknown, the parameters of camera groups: the Jacobian J_k, the rows of 36 doubles, the groups' blocks and their fold over a
group's frames (:func:`group_fold`), the three-pass matvec, the conjugate gradients over 6 F + 8 G unknowns, the candidate and the
loop.  :func:`dense_run` is an independent form: the full Jacobian over poses, intrinsics and points and numpy.linalg.solve.
Also the scenes and runs the CPU and GPU tests share."""
from __future__ import annotations

import numpy as np

from tests import bundle_ref as BR
from tests import pose_ref as PR
from tests import triangulation_ref as TR

OBS_DOUBLES = 36      # PRAM_BAC_OBS_DOUBLES
NK = 8                # PRAM_BAC_GROUP_PARAMS
N_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8}      # by PRAM_CAM_* id
N_FOCAL = {0: 1, 1: 2, 2: 1, 3: 1, 4: 2}
_IGN = dict(all="ignore")
_J20 = list(range(12)) + list(range(28, 36))      # the columns of bundle_ref's row inside the row of 36


# ---------------------------------------------------------------- the camera model's Jacobian
def unify(model: int, k) -> np.ndarray:
    return np.asarray(PR.unify(int(model), np.asarray(k, dtype=np.float64)), dtype=np.float64).reshape(8)


def param_jac(model: int, c, u, v, ud, vd, r2) -> np.ndarray:
    """camera.h's cam_param_jac -> [n, 2, 8]: d residual / d (the model's own parameters), zero padded.  c: the unified camera [8]
    (fx, fy, cx, cy, k1, k2, p1, p2) or [n, 8]."""
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), (np.shape(u)[0], 8))
    fx, fy = c[:, 0], c[:, 1]
    J = np.zeros((np.shape(u)[0], 2, 8))
    one = np.ones_like(u)
    k1, k2 = (fx * u * r2, fy * v * r2), (fx * u * r2 * r2, fy * v * r2 * r2)
    cols = {0: [(ud, vd), (one, 0), (0, one)], 1: [(ud, 0), (0, vd), (one, 0), (0, one)], 2: [(ud, vd), (one, 0), (0, one), k1],
            3: [(ud, vd), (one, 0), (0, one), k1, k2],
            4: [(ud, 0), (0, vd), (one, 0), (0, one), k1, k2, (fx * (2.0 * u * v), fy * (r2 + 2.0 * v * v)),
                (fx * (r2 + 2.0 * u * u), fy * (2.0 * u * v))]}[int(model)]
    for a, (x, y) in enumerate(cols):
        J[:, 0, a], J[:, 1, a] = x, y
    return J


# ---------------------------------------------------------------- the problem
class GroupProblem:
    """bundle_ref's Problem with the group tables of pram_bac_begin: frm_grp [F], the CSR, the groups' parameters [G, 8] and the
    masks as bac_setup_kernel makes them (the caller's bits, the parameters the model does not have, everything for a group
    without observations)."""

    def __init__(self, pr: BR.Problem, frm_grp, grp_params, grp_mask):
        self.pr = pr
        self.frm_grp = np.asarray(frm_grp, dtype=np.int64)
        self.G = int(self.frm_grp.max()) + 1
        order = np.argsort(self.frm_grp, kind="stable")
        self.grp_off = np.zeros(self.G + 1, dtype=np.int64)
        self.grp_off[1:] = np.cumsum(np.bincount(self.frm_grp, minlength=self.G))
        self.grp_frame = order
        self.k0 = np.array(grp_params, dtype=np.float64).reshape(self.G, NK)
        self.mask_in = np.asarray(grp_mask, dtype=np.int64).reshape(self.G)
        self.model = np.array([int(pr.cam_model[self.frames_of(q)[0]]) for q in range(self.G)])
        for q in range(self.G):
            assert (pr.cam_model[self.frames_of(q)] == self.model[q]).all()
        cnt = np.diff(pr.frm_off)
        self.n_obs = np.array([int(cnt[self.frames_of(q)].sum()) for q in range(self.G)])
        absent = np.array([255 & ~((1 << N_PARAMS[m]) - 1) for m in self.model.tolist()])
        self.gmask = np.where(self.n_obs > 0, (self.mask_in & 255) | absent, 255)
        self.F, self.P, self.O = pr.F, pr.P, pr.O

    def frames_of(self, q: int) -> np.ndarray:
        return self.grp_frame[self.grp_off[q]:self.grp_off[q + 1]]

    def frozen_bits(self) -> np.ndarray:
        return ((self.gmask[:, None] >> np.arange(NK)[None]) & 1).astype(bool)

    def set_cameras(self, k) -> np.ndarray:
        """The per-frame parameters from the groups' (bac_expand_kernel) into the problem's observation model -> cam [F, 8] unified."""
        cam = np.stack([unify(self.model[q], k[q]) for q in self.frm_grp.tolist()])
        self.pr.track.cam = cam[self.pr.obs_frame]
        return cam


def group_fold(values, frames) -> np.ndarray:
    """The blocked order of BR.BLOCK over a group's list of frames: each block's rows added to 0.0 in ascending order, the block
    partials added to 0.0 in ascending order."""
    values = np.asarray(values, dtype=np.float64)
    total = np.zeros(values.shape[1:])
    for a in range(0, len(frames), BR.BLOCK):
        s = np.zeros(values.shape[1:])
        for f in np.asarray(frames[a:a + BR.BLOCK]).tolist():
            s = s + values[f]
        total = total + s
    return total


def _dot8(a, b):
    s = np.zeros(a.shape[0])
    for k in range(NK):
        s = s + a[:, k] * b[:, k]
    return s


def dot_total(af, bf, ag, bg) -> float:
    """A dot product over the 6 F + 8 G unknowns: the frames' blocked sum, then the groups', the two added frames first."""
    return BR.blocked_sum(BR._dot6(af, bf)) + BR.blocked_sum(_dot8(ag, bg))


# ---------------------------------------------------------------- linearise
def linearise(gp: GroupProblem, table, xyz, k, loss_scale: float = 1.0):
    """-> J [O, 36] (sqrt(w) J_c [2][6], sqrt(w) J_k [2][8], sqrt(w) J_p [2][3], sqrt(w) r [2]), ok [O], extras (the unweighted
    J_k among them)."""
    pr = gp.pr
    cam = gp.set_cameras(k)
    J20, ok, ex = BR.linearise(pr, table, xyz, loss_scale)
    T, X = table[pr.obs_frame], xyz[pr.obs_point]
    with np.errstate(**_IGN):
        sw = np.sqrt(1.0 / (1.0 + ex["s"]))
        Y0 = T[:, 0] * X[:, 0] + T[:, 1] * X[:, 1] + T[:, 2] * X[:, 2]
        Y1 = T[:, 3] * X[:, 0] + T[:, 4] * X[:, 1] + T[:, 5] * X[:, 2]
        u, v = (Y0 + T[:, 9]) / ex["z"], (Y1 + T[:, 10]) / ex["z"]
        c = cam[pr.obs_frame]
        ud, vd = PR.distort(u, v, c[:, 4], c[:, 5], c[:, 6], c[:, 7])
        Jk = np.zeros((pr.O, 2, NK))
        og = gp.frm_grp[pr.obs_frame]
        for q in range(gp.G):
            m = og == q
            if m.any():
                Jk[m] = param_jac(gp.model[q], c[m], u[m], v[m], ud[m], vd[m], u[m] * u[m] + v[m] * v[m])
        frozen = gp.frozen_bits()[og]
        J = np.zeros((pr.O, OBS_DOUBLES))
        J[:, _J20] = J20
        for i in range(2):
            J[:, 12 + i * NK:12 + (i + 1) * NK] = np.where(frozen, 0.0, sw[:, None] * Jk[:, i])
    J[~ok] = 0.0
    return J, ok, {**ex, "Jk": Jk, "sw": sw}


# ---------------------------------------------------------------- blocks
def _sum_terms(j, N: int, OFF: int, V, g):
    """frame_terms of bundle.hip per observation: N (N + 1) / 2 + 3 N columns."""
    jc0, jc1, jp = j[:, OFF:OFF + N], j[:, OFF + N:OFF + 2 * N], j[:, 28:34]
    r0, r1 = j[:, 34], j[:, 35]
    W = np.stack([np.stack([jc0[:, a] * jp[:, k] + jc1[:, a] * jp[:, 3 + k] for k in range(3)], 1) for a in range(N)], 1)
    WV = np.stack([BR._vinv_mul(V, W[:, a]) for a in range(N)], 1)
    cols = []
    for a in range(N):
        for c in range(a, N):
            cols.append((jc0[:, a] * jc0[:, c] + jc1[:, a] * jc1[:, c]) - (WV[:, a, 0] * W[:, c, 0] + WV[:, a, 1] * W[:, c, 1] + WV[:, a, 2] * W[:, c, 2]))
    cols += [jc0[:, a] * jc0[:, a] + jc1[:, a] * jc1[:, a] for a in range(N)]
    cols += [jc0[:, a] * r0 + jc1[:, a] * r1 for a in range(N)]
    cols += [WV[:, a, 0] * g[:, 0] + WV[:, a, 1] * g[:, 1] + WV[:, a, 2] * g[:, 2] for a in range(N)]
    return np.stack(cols, 1)


def group_blocks(gp: GroupProblem, J, Vinv, g_p, lam: float):
    """-> the groups' blocks [G, 36] (damped; a frozen parameter's diagonal 1), diag U_k [G, 8], b_k [G, 8], and the frames'
    partial sums [F, 60]."""
    pr = gp.pr
    part = np.zeros((pr.F, 60))
    for f in range(pr.F):
        a0, a1 = pr.frm_off[f], pr.frm_off[f + 1]
        if a1 > a0:
            p = pr.obs_point[a0:a1]
            part[f] = BR.frame_sum(_sum_terms(J[a0:a1], NK, 12, Vinv[p], g_p[p]))
    S, dU, b = np.zeros((gp.G, 36)), np.zeros((gp.G, NK)), np.zeros((gp.G, NK))
    for q in range(gp.G):
        tot = group_fold(part, gp.frames_of(q))
        e = 0
        for a in range(NK):
            for c in range(a, NK):
                v = tot[e]
                if a == c:
                    v = 1.0 if (gp.gmask[q] >> a) & 1 else v + lam * tot[36 + a]
                S[q, e] = v
                e += 1
        dU[q], b[q] = tot[36:44], tot[52:60] - tot[44:52]
    return S, dU, b, part


def _sym8(Su):
    M = np.zeros((NK, NK))
    e = 0
    for a in range(NK):
        for c in range(a, NK):
            M[a, c] = M[c, a] = Su[e]
            e += 1
    return M


def chol_solve8(A, b):
    """A x = b by Cholesky in chol_solve8's order; None when a pivot is not positive or x is not finite."""
    L = np.zeros((NK, NK))
    for i in range(NK):
        for k in range(i + 1):
            s = 0.0
            for j in range(k):
                s = s + L[i, j] * L[k, j]
            s = A[k, i] - s
            if i == k:
                if not s > 0.0:
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, k] = s / L[k, k]
    y, x = np.zeros(NK), np.zeros(NK)
    for i in range(NK):
        s = 0.0
        for j in range(i):
            s = s + L[i, j] * y[j]
        y[i] = (b[i] - s) / L[i, i]
    for i in range(NK - 1, -1, -1):
        s = 0.0
        for j in range(i + 1, NK):
            s = s + L[j, i] * x[j]
        x[i] = (y[i] - s) / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def precond8(S, r):
    z = np.zeros_like(r)
    for q in range(r.shape[0]):
        x = chol_solve8(_sym8(S[q]), r[q])
        z[q] = r[q] if x is None else x
    return z


# ---------------------------------------------------------------- the matvec, three passes
def _t(gp: GroupProblem, J, v, vg):
    pr = gp.pr
    vf, wg = v[pr.obs_frame], vg[gp.frm_grp[pr.obs_frame]]
    t0, t1 = np.zeros(pr.O), np.zeros(pr.O)
    for a in range(6):
        t0 = t0 + J[:, a] * vf[:, a]
        t1 = t1 + J[:, 6 + a] * vf[:, a]
    for a in range(NK):
        t0 = t0 + J[:, 12 + a] * wg[:, a]
        t1 = t1 + J[:, 20 + a] * wg[:, a]
    return t0, t1


def mv_points(gp: GroupProblem, J, Vinv, v, vg):
    """Per point: V^-1 sum J_p^T (J_c v_f + J_k v_g) -> (y [P, 3], the sums before V^-1)."""
    pr = gp.pr
    t0, t1 = _t(gp, J, v, vg)
    terms = np.stack([J[:, 28 + c] * t0 + J[:, 31 + c] * t1 for c in range(3)], 1)
    acc = np.zeros((pr.P, 3))
    for p in range(pr.P):
        o = pr.pt_obs[pr.pt_off[p]:pr.pt_off[p + 1]]
        if len(o):
            acc[p] = TR.wave_sum(terms[o])
    return BR._vinv_mul(Vinv, acc), acc


def matvec(gp: GroupProblem, J, Vinv, dU, dUg, lam: float, v, vg):
    """(q_f [F, 6], q_g [G, 8]) = S (v, v_g)."""
    pr = gp.pr
    y, _ = mv_points(gp, J, Vinv, v, vg)
    t0, t1 = _t(gp, J, v, vg)
    yo = y[pr.obs_point]
    t0 = t0 - (J[:, 28] * yo[:, 0] + J[:, 29] * yo[:, 1] + J[:, 30] * yo[:, 2])
    t1 = t1 - (J[:, 31] * yo[:, 0] + J[:, 32] * yo[:, 1] + J[:, 33] * yo[:, 2])
    terms = np.stack([J[:, a] * t0 + J[:, 6 + a] * t1 for a in range(6)] + [J[:, 12 + a] * t0 + J[:, 20 + a] * t1 for a in range(NK)], 1)
    q, part = np.zeros((pr.F, 6)), np.zeros((pr.F, NK))
    for f in range(pr.F):
        a0, a1 = pr.frm_off[f], pr.frm_off[f + 1]
        tot = BR.frame_sum(terms[a0:a1]) if a1 > a0 else np.zeros(14)
        frozen = ((pr.fmask[f] >> np.arange(6)) & 1).astype(bool)
        q[f] = np.where(frozen, v[f], tot[:6] + lam * dU[f] * v[f])
        part[f] = tot[6:]
    qg = np.zeros((gp.G, NK))
    fz = gp.frozen_bits()
    for g in range(gp.G):
        tot = group_fold(part, gp.frames_of(g))
        qg[g] = np.where(fz[g], vg[g], tot + lam * dUg[g] * vg[g])
    return q, qg


def pcg(gp: GroupProblem, J, Vinv, S, Sg, dU, dUg, b, bg, lam: float, cg_iters: int, cg_tol: float):
    """-> (x [F, 6], x_g [G, 8], iterations, trace)."""
    x, xg, r, rg = np.zeros_like(b), np.zeros_like(bg), b.copy(), bg.copy()
    z, zg = BR.precond(S, r), precond8(Sg, rg)
    p, pg = z.copy(), zg.copy()
    rz, bb = dot_total(r, z, rg, zg), dot_total(r, r, rg, rg)
    tr = {"stop": [], "fail": 0, "first": {"z": z.copy(), "zg": zg.copy(), "rz": rz, "bb": bb}}
    it = 0
    if not bb > 0.0:
        return x, xg, it, tr
    for _ in range(cg_iters):
        q, qg = matvec(gp, J, Vinv, dU, dUg, lam, p, pg)
        pap = dot_total(p, q, pg, qg)
        if it == 0:
            tr["first"].update(q=q.copy(), qg=qg.copy(), pap=pap)
        with np.errstate(**_IGN):
            alpha = rz / pap
        if not pap > 0.0 or not np.isfinite(alpha):
            tr["fail"] += 1
            break
        x, xg = x + alpha * p, xg + alpha * pg
        r, rg = r - alpha * q, rg - alpha * qg
        z, zg = BR.precond(S, r), precond8(Sg, rg)
        rz_new, rr = dot_total(r, z, rg, zg), dot_total(r, r, rg, rg)
        if it == 0:
            tr["first"].update(x1=x.copy(), xg1=xg.copy(), rr1=rr)
        with np.errstate(**_IGN):
            beta = rz_new / rz
        rz = rz_new
        it += 1
        tr["stop"].append(float(np.sqrt(rr) / (cg_tol * np.sqrt(bb))))
        if np.sqrt(rr) <= cg_tol * np.sqrt(bb) or not np.isfinite(beta):
            break
        p, pg = z + beta * p, zg + beta * pg
    return x, xg, it, tr


# ---------------------------------------------------------------- the loop
def candidate_params(gp: GroupProblem, k, xg):
    """-> (k + d_k, a group whose step is 0 keeping its bits; bad: a focal length not finite or not above 0)."""
    kc = np.where(xg == 0.0, k, k + xg)
    bad = False
    for q in range(gp.G):
        f = kc[q, :N_FOCAL[gp.model[q]]]
        bad = bad or not (np.isfinite(f).all() and (f > 0.0).all())
    return kc, bad


def cost(gp: GroupProblem, table, xyz, k, loss_scale: float = 1.0) -> float:
    gp.set_cameras(k)
    return BR.cost(gp.pr, table, xyz, loss_scale)


def lm_step(gp: GroupProblem, table, xyz, k, J, ok, lam: float, p: dict):
    pr = gp.pr
    J20 = J[:, _J20]
    Vinv, g_p, good = BR.point_blocks(pr, J20, ok, lam)
    S, dU, b = BR.frame_blocks(pr, J20, Vinv, g_p, lam)
    Sg, dUg, bg, part = group_blocks(gp, J, Vinv, g_p, lam)
    x, xg, n_cg, tr = pcg(gp, J, Vinv, S, Sg, dU, dUg, b, bg, lam, p["cg_iters"], p["cg_tol"])
    _, acc = mv_points(gp, J, Vinv, x, xg)
    xyz_c = xyz - BR._vinv_mul(Vinv, g_p + acc)
    table_c = np.stack([BR.rodrigues_update(table[f], x[f]) for f in range(pr.F)])
    kc, bad = candidate_params(gp, k, xg)
    tr.update(Vinv=Vinv, gp=g_p, S=S, dU=dU, b=b, Sg=Sg, dUg=dUg, bg=bg, part=part)
    return table_c, xyz_c, kc, bad, x, xg, n_cg, tr, good


def run(gp: GroupProblem, **params) -> dict:
    """The whole adjustment -> table, xyz, params [G, 8], the report's numbers, the filter and the margins of every decision."""
    p = {**BR.DEFAULTS, **params}
    pr = gp.pr
    table, xyz, k, lam = pr.table.copy(), pr.xyz.copy(), gp.k0.copy(), float(p["lam0"])
    c0 = c = cost(gp, table, xyz, k, p["loss_scale"])
    accepted, cg_counts, accept_margin, cg_margin, fails = [], [], [], [], 0
    reason, good, first = "max_iters", np.ones(pr.P, dtype=bool), None
    J = ok = None
    moved = np.zeros(pr.F, dtype=bool)
    for it in range(p["max_iters"]):
        if J is None:
            J, ok, _ = linearise(gp, table, xyz, k, p["loss_scale"])
        table_c, xyz_c, kc, bad, x, xg, n_cg, tr, good = lm_step(gp, table, xyz, k, J, ok, lam, p)
        if first is None:
            first = {"J": J.copy(), "ok": ok.copy(), "x": x.copy(), "xg": xg.copy(), **tr}
        c1 = float("nan") if bad else cost(gp, table_c, xyz_c, kc, p["loss_scale"])
        acc = bool(c1 < c)
        accepted.append(acc); cg_counts.append(n_cg); fails += tr["fail"]
        accept_margin.append(abs(c1 - c) / c if np.isfinite(c1) and c > 0 else np.inf)
        cg_margin.append(min([abs(s - 1.0) for s in tr["stop"]], default=np.inf))
        if acc:
            rel = (c - c1) / c
            table, xyz, k, c = table_c, xyz_c, kc, c1
            moved |= np.any(x != 0.0, axis=1)
            lam = max(lam * 0.1, 1e-15)
            J = None
            if rel < p["ftol"]:
                reason = "ftol"
                break
        else:
            lam = lam * 10.0
    gp.set_cameras(k)
    flt = BR.filter_points(pr, table, xyz, p["max_reproj_error"], p["min_tri_angle"], p["loss_scale"])
    return {"table": table, "xyz": xyz, "params": k, "initial_cost": c0, "final_cost": c, "accepted": np.array(accepted, dtype=bool),
            "cg_iterations": np.array(cg_counts, dtype=np.int64), "lam": lam, "termination": reason, "moved": moved, "solvable": good,
            "cg_breakdowns": fails, "first": first, "filter": flt,
            "margins": {"accept": np.array(accept_margin), "cg": np.array(cg_margin)}}


# ---------------------------------------------------------------- the independent dense form
def dense_jacobian(gp: GroupProblem, table, xyz, k, loss_scale: float = 1.0):
    """-> (Jd [2 O, 6 F + 8 G + 3 P], rd [2 O]) of the weighted problem, frozen columns zero."""
    pr = gp.pr
    J, ok, _ = linearise(gp, table, xyz, k, loss_scale)
    nc = 6 * pr.F + NK * gp.G
    Jd, rd = np.zeros((2 * pr.O, nc + 3 * pr.P)), np.zeros(2 * pr.O)
    for o in range(pr.O):
        f, pt = pr.obs_frame[o], pr.obs_point[o]
        g = gp.frm_grp[f]
        for i in range(2):
            Jd[2 * o + i, 6 * f:6 * f + 6] = J[o, i * 6:i * 6 + 6]
            Jd[2 * o + i, 6 * pr.F + NK * g:6 * pr.F + NK * g + NK] = J[o, 12 + i * NK:12 + (i + 1) * NK]
            Jd[2 * o + i, nc + 3 * pt:nc + 3 * pt + 3] = J[o, 28 + i * 3:31 + i * 3]
            rd[2 * o + i] = J[o, 34 + i]
    weighted = np.bincount(pr.obs_point[ok], minlength=pr.P)
    for pt in np.nonzero(weighted < 2)[0].tolist():
        Jd[:, nc + 3 * pt:nc + 3 * pt + 3] = 0.0
    return Jd, rd


def dense_step(gp: GroupProblem, table, xyz, k, lam: float, loss_scale: float = 1.0):
    Jd, rd = dense_jacobian(gp, table, xyz, k, loss_scale)
    H, g = Jd.T @ Jd, Jd.T @ rd
    dg = np.diag(H).copy()
    H = H + lam * np.diag(dg)
    dead = dg == 0.0
    H[dead, dead] = 1.0
    return np.linalg.solve(H, -g), H, g


def dense_run(gp: GroupProblem, **params) -> dict:
    """Levenberg-Marquardt with the device's accept rule on the dense normal equations over poses, intrinsics and points."""
    p = {**BR.DEFAULTS, **params}
    pr = gp.pr
    table, xyz, k, lam = pr.table.copy(), pr.xyz.copy(), gp.k0.copy(), float(p["lam0"])
    c = c0 = cost(gp, table, xyz, k, p["loss_scale"])
    n, nc = 0, 6 * pr.F + NK * gp.G
    for _ in range(p["max_iters"]):
        d, _, _ = dense_step(gp, table, xyz, k, lam, p["loss_scale"])
        table_c = np.stack([BR.rodrigues_update(table[f], d[6 * f:6 * f + 6]) for f in range(pr.F)])
        kc, bad = candidate_params(gp, k, d[6 * pr.F:nc].reshape(gp.G, NK))
        xyz_c = xyz + d[nc:].reshape(-1, 3)
        c1 = float("nan") if bad else cost(gp, table_c, xyz_c, kc, p["loss_scale"])
        n += 1
        if c1 < c:
            rel = (c - c1) / c
            table, xyz, k, c, lam = table_c, xyz_c, kc, c1, max(lam * 0.1, 1e-15)
            if rel < p["ftol"]:
                break
        else:
            lam *= 10.0
    return {"table": table, "xyz": xyz, "params": k, "initial_cost": c0, "final_cost": c, "iterations": n}


def reduced_dense(gp: GroupProblem, J, Vinv, lam: float) -> np.ndarray:
    """The reduced matrix [6 F + 8 G, 6 F + 8 G] written out: U + lam diag U - W V^-1 W^T, a frozen parameter's diagonal 1."""
    pr = gp.pr
    nc = 6 * pr.F + NK * gp.G
    A, Wd = np.zeros((2 * pr.O, nc)), np.zeros((nc, 3 * pr.P))
    for o in range(pr.O):
        f = pr.obs_frame[o]
        g = gp.frm_grp[f]
        for i in range(2):
            A[2 * o + i, 6 * f:6 * f + 6] = J[o, i * 6:i * 6 + 6]
            A[2 * o + i, 6 * pr.F + NK * g:6 * pr.F + NK * g + NK] = J[o, 12 + i * NK:12 + (i + 1) * NK]
    Ud = A.T @ A
    Ud = Ud + lam * np.diag(np.diag(Ud))
    Jp = np.zeros((2 * pr.O, 3 * pr.P))
    for o in range(pr.O):
        pt = pr.obs_point[o]
        for i in range(2):
            Jp[2 * o + i, 3 * pt:3 * pt + 3] = J[o, 28 + i * 3:31 + i * 3]
    Wd = A.T @ Jp
    Vd = np.zeros((3 * pr.P, 3 * pr.P))
    for pt in range(pr.P):
        v = Vinv[pt]
        Vd[3 * pt:3 * pt + 3, 3 * pt:3 * pt + 3] = [[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]]
    S = Ud - Wd @ Vd @ Wd.T
    for f in range(pr.F):
        for a in range(6):
            if (pr.fmask[f] >> a) & 1:
                S[6 * f + a, 6 * f + a] = 1.0
    fz = gp.frozen_bits()
    for g in range(gp.G):
        for a in range(NK):
            if fz[g, a]:
                S[6 * pr.F + NK * g + a, 6 * pr.F + NK * g + a] = 1.0
    return S


# ---------------------------------------------------------------- scenes with groups laid over them
# The runs the GPU test makes are short on purpose.  The reduced system with the intrinsics in it is badly conditioned and its
# preconditioner leaves the coupling of a pose and its camera out, so the conjugate gradients run long, and a long run of them
# multiplies the last bits it starts from: with the default budget of 60 iterations the device and numpy, which agree on every
# single-pass quantity, end 1e-5 degrees apart after three steps (measured; profiles/bundle_intrinsics_parity.md), and so does
# numpy against itself when its input moves by one part in 1e15.  A budget of 12 keeps what the device's sin, cos and log1p differ
# by from numpy's at the size it enters with.  Three steps run every kernel; the first solve of every run stops on its tolerance,
# the later ones on the budget; the ring's run (four steps of 16) has a rejected step and the accepted one after it.
RUN_ITERS = 3
RUN_PARAMS = {"max_iters": RUN_ITERS, "cg_iters": 12}
RING_PARAMS = {"max_iters": 4, "cg_iters": 16}
FOCAL, PP, EXTRA = ({0: (0,), 1: (0, 1), 2: (0,), 3: (0,), 4: (0, 1)}, {0: (1, 2), 1: (2, 3), 2: (1, 2), 3: (1, 2), 4: (2, 3)},
                    {0: (), 1: (), 2: (3,), 3: (3, 4), 4: (4, 5, 6, 7)})


def flag_mask(model: int, focal: bool, pp: bool, extra: bool) -> int:
    free = (FOCAL[model] if focal else ()) + (PP[model] if pp else ()) + (EXTRA[model] if extra else ())
    return 255 & ~sum(1 << a for a in free)


def with_cameras(s: dict, cameras) -> dict:
    """A copy of a scene with other cameras (one tuple per frame): the keypoints stay, the table and the normalisations follow."""
    out = dict(s)
    rows = [PR.camera_row(c) for c in cameras]
    out["cameras"] = list(cameras)
    out["cam_model"], out["cam_params"] = np.array([r[0] for r in rows], dtype=np.int32), np.stack([r[1] for r in rows])
    out["table"] = TR.frame_table(out["qvec"], out["tvec"], out["cam_model"], out["cam_params"])
    out["norm0"] = TR.normalize(out["keypoints"], out["frame_off"], out["cam_model"], out["cam_params"], 0.0)
    out["norm05"] = TR.normalize(out["keypoints"], out["frame_off"], out["cam_model"], out["cam_params"], 0.5)
    return out


def group_problem(s: dict, model: dict, frozen, frm_grp, flags=(True, False, True), masks=None) -> tuple:
    """-> (GroupProblem, the observation tables) for a scene whose frames of a group share one camera."""
    pr, tabs = BR.problem_of(s, model, frozen=frozen)
    frm_grp = np.asarray(frm_grp, dtype=np.int64)
    G = int(frm_grp.max()) + 1
    first = [int(np.nonzero(frm_grp == q)[0][0]) for q in range(G)]
    prm = np.zeros((G, NK))
    mask = np.zeros(G, dtype=np.int64)
    for q, f in enumerate(first):
        x = np.asarray(s["cameras"][f][3], dtype=np.float64)
        prm[q, :x.shape[0]] = x
        mask[q] = flag_mask(int(s["cam_model"][f]), *flags)
    if masks is not None:
        mask = mask | np.asarray(masks, dtype=np.int64)
    return GroupProblem(pr, frm_grp, prm, mask), tabs


def arc_scene(cameras, n_points: int = 120, noise: float = 0.0, seed: int = 1, visible: float = 0.7, outliers: float = 0.0) -> dict:
    """Frames on an arc that look at the origin through ``cameras`` (one tuple per frame), points in a box, each seen by a frame
    with probability ``visible``; keypoints with Gaussian noise of ``noise`` pixels; a share ``outliers`` of them displaced by 20
    to 60 pixels."""
    rng = np.random.RandomState(seed)
    F = len(cameras)
    ang = np.deg2rad(np.linspace(-50.0, 50.0, F))
    centres = [np.array([8.0 * np.sin(a), 1.2 * np.cos(3 * a), -8.0 * np.cos(a) + 0.8 * np.sin(2 * a)]) for a in ang]
    s = TR._base(list(cameras), centres, [np.array([0.3 * np.sin(5 * a), 0.2 * np.cos(4 * a), 0.0]) for a in ang])
    xyz = rng.uniform([-2.2, -1.6, -2.0], [2.2, 1.6, 2.0], size=(n_points, 3))
    kps, where = [[] for _ in range(F)], {}
    for f in range(F):
        px, z = TR.project(s, f, xyz)
        for p in rng.permutation(n_points).tolist():
            if rng.uniform() < visible and z[p] > 0 and 2 <= px[p, 0] < TR.WIDTH - 2 and 2 <= px[p, 1] < TR.HEIGHT - 2:
                e = rng.normal(size=2) * noise
                if rng.uniform() < outliers:
                    e = e + rng.uniform(20.0, 60.0) * np.array([np.cos(t := rng.uniform(0, 2 * np.pi)), np.sin(t)])
                kps[f].append(tuple(px[p] - 0.5 + e))
                where[(f, p)] = len(kps[f]) - 1
    s.update(pairs=np.zeros((0, 2), dtype=np.int64), matches=[], xyz=xyz, where=where, noise=noise)
    return TR._finish(s, kps)


def _scaled(cam, focal: float = 1.0, k1=None):
    name, w, h, prm = cam
    prm = np.array(prm, dtype=np.float64)
    m = PR.camera_row(cam)[0]
    prm[list(FOCAL[int(m)])] *= focal
    if k1 is not None and EXTRA[int(m)]:
        prm[EXTRA[int(m)][0]] = k1
    return (name, w, h, prm.tolist())


_recovery: dict = {}


def recovery_case(noise: float = 0.0, outliers: float = 0.0, seed: int = 21, n_frames: int = 12, n_points: int = 120) -> dict:
    """The planted scene: a RADIAL camera shared by most frames and a SIMPLE_RADIAL one by the last three; the adjustment starts
    from focal lengths 5 % off, k1 = 0 and perturbed poses.  -> truth (scene), scene (the start), model, frozen, frm_grp."""
    key = (noise, outliers, seed, n_frames, n_points)
    if key in _recovery:
        return _recovery[key]
    A = ("RADIAL", TR.WIDTH, TR.HEIGHT, [525.0, 319.0, 241.0, -0.06, 0.02])
    B = ("SIMPLE_RADIAL", TR.WIDTH, TR.HEIGHT, [508.0, 321.0, 238.0, -0.05])
    cams = [A] * (n_frames - 3) + [B] * 3
    truth = arc_scene(cams, n_points=n_points, noise=noise, seed=seed, outliers=outliers)
    start = with_cameras(truth, [_scaled(c, 1.05, 0.0) for c in cams])
    q, t = BR.perturb_poses(start, 0.3, 0.05, seed=seed + 1, keep=(0,))
    start = BR.with_poses(start, q, t)
    model = BR.planted_model(truth)
    frozen = np.zeros(n_frames, dtype=np.int64)
    frozen[0], frozen[1] = 63, 1 << 3
    frm_grp = np.array([0] * (n_frames - 3) + [1] * 3)
    _recovery[key] = {"truth": truth, "scene": start, "model": model, "frozen": frozen, "frm_grp": frm_grp, "params": {"max_iters": 40}}
    return _recovery[key]


def one_camera_ring(cam=TR.CAMERAS[4]) -> dict:
    """bundle_ref's ring case (70 frames, a track of 65 entries) seen through ONE camera: a group of 70 frames, which crosses
    BR.BLOCK.  The scene is rebuilt with that camera, so its keypoints are consistent with it."""
    s = BR.gpu_case("ring")["truth"]
    rng = np.random.RandomState(5)
    F, lengths = s["n_frames"], s["lengths"]
    one = TR._base([cam] * F, [s["table"][f, 12:15] for f in range(F)], [np.zeros(3)] * F)
    kps, where = [[] for _ in range(F)], {}
    for f in range(F):
        px, z = TR.project(one, f, s["xyz"])
        for p in rng.permutation(len(lengths)).tolist():
            if f < lengths[p]:
                kps[f].append(tuple(px[p] - 0.5 + rng.uniform(-0.3, 0.3, size=2)))
                where[(f, p)] = len(kps[f]) - 1
    one.update(pairs=np.zeros((0, 2), dtype=np.int64), matches=[], xyz=s["xyz"], where=where, lengths=lengths, noise=0.3)
    return TR._finish(one, kps)


def _case_models() -> dict:
    """tri_scene's special case: five groups by the default grouping (frames f, f + 5, ...: not contiguous), one per camera model,
    3 / 4 / 4 / 5 / 8 parameters; frame 11 has no keypoint.  Focal lengths and the extra parameters free."""
    c = BR.gpu_case("special")
    grp = np.arange(c["scene"]["n_frames"]) % 5
    return {**c, "frm_grp": grp, "flags": (True, False, True), "masks": None, "params": dict(RUN_PARAMS)}


def _case_models_pp() -> dict:
    """The same with the principal point free too and, in the OPENCV group, p1 (bit 6) frozen by the per-group mask."""
    c = _case_models()
    return {**c, "flags": (True, True, True), "masks": np.array([0, 0, 0, 0, 1 << 6])}


def _case_ring() -> dict:
    """One group of 70 frames (a track of 65 entries); the frames from 30 on are pose-frozen."""
    c = BR.gpu_case("ring")
    s = one_camera_ring()
    q, t = BR.perturb_poses(s, 0.3, 0.05, seed=4, keep=(0,))
    sp = BR.with_poses(s, q, t)
    start = with_cameras(sp, [_scaled(TR.CAMERAS[4], 1.02)] * s["n_frames"])
    return {"scene": start, "truth": s, "model": BR.planted_model(s), "frozen": c["frozen"], "frm_grp": np.zeros(s["n_frames"], dtype=np.int64),
            "flags": (True, False, True), "masks": None, "params": dict(RING_PARAMS)}


def _case_frames() -> dict:
    """frames_scene (frames of 0, 1, 63, 64, 65, 257 and 200 observations over the five models; odd and even frames would mix
    models, so the groups are the models'): frames 0 and 5, 1 and 6, then three groups of one frame.  Frames 5 and 6 are
    pose-frozen and frame 0 has no observation, so every frame of the first group is pose-frozen."""
    c = BR.gpu_case("frames")
    F = c["scene"]["n_frames"]
    return {**c, "frm_grp": np.arange(F) % 5, "flags": (True, False, True), "masks": None, "params": dict(RUN_PARAMS)}


def _case_split() -> dict:
    """One camera over the recovery scene's frames, split by hand into odd and even frames (two groups that are not contiguous),
    with a third group of one frame whose every parameter is pose-frozen, and a fourth whose only frame has no observation."""
    cam = TR.CAMERAS[3]
    s = arc_scene([cam] * 9 + [TR.CAMERAS[2]], n_points=60, noise=0.3, seed=31)
    s["where"] = {(f, p): k for (f, p), k in s["where"].items() if f != 9}      # frame 9 (its own camera) is seen by no point
    q, t = BR.perturb_poses(s, 0.3, 0.05, seed=32, keep=(0, 8))
    sp = BR.with_poses(s, q, t)
    start = with_cameras(sp, [_scaled(c, 1.03) for c in s["cameras"]])
    frozen = np.zeros(10, dtype=np.int64)
    frozen[0], frozen[1], frozen[8] = 63, 1 << 3, 63
    grp = np.array([0, 1, 0, 1, 0, 1, 0, 1, 2, 3])
    return {"scene": start, "truth": s, "model": BR.planted_model(s), "frozen": frozen, "frm_grp": grp, "flags": (True, True, True), "masks": None,
            "params": dict(RUN_PARAMS)}


GPU_RUNS = {"models": _case_models, "models_pp": _case_models_pp, "ring": _case_ring, "frames": _case_frames, "split": _case_split}
_cases: dict = {}
_runs: dict = {}


def gpu_case(name: str) -> dict:
    if name not in _cases:
        c = dict(GPU_RUNS[name]())
        c["problem"], c["tables"] = group_problem(c["scene"], c["model"], c["frozen"], c["frm_grp"], c["flags"], c["masks"])
        _cases[name] = c
    return _cases[name]


def gpu_run(name: str) -> dict:
    if name not in _runs:
        c = gpu_case(name)
        _runs[name] = run(c["problem"], **c["params"])
    return _runs[name]
