"""CPU: the numpy restatement of the bundle adjustment with camera groups (tests/bundle_intr_ref.py) against central differences,
the dense reduced matrix, a dense solve of the full normal equations and scipy; what it recovers on a planted scene whose focal
lengths start 5 % off; the margins that make the discrete decisions of the GPU test's runs exact; and the host side of
pram_amd.localization.bundle's refine flags and of the mapper's pass-through with ops replaced by the restatement.

The runs of bundle_intr_ref.GPU_RUNS and what each is there for:
  models     tri_scene's twelve frames in five groups by the default grouping, one per camera model (3 / 4 / 4 / 5 / 8 parameters),
             the frames of a group not contiguous (f, f + 5, ...); a frame without a keypoint; focal lengths and distortion free;
  models_pp  the same with the principal point free too, and p1 of the OPENCV group frozen by the per-group mask;
  ring       one OPENCV camera over the ring's 70 frames: a group that crosses PRAM_BA_BLOCK, a track of 65 entries;
  frames     frames of 0, 1, 63, 64, 65, 257 and 200 observations; groups of one frame; a group whose frames are both pose-frozen;
  split      one camera split into odd and even frames (two groups, not contiguous), a group of one frame that is pose-frozen,
             and a group without observations, which is frozen by the entry."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import bundle_intr_ref as IR
from tests import bundle_ref as BR
from tests import pose_ref as PR
from tests import triangulation_ref as TR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_bac_workspace_bytes", "pram_bac_layout", "pram_bac_begin", "pram_bac_iterate", "pram_bac_finish")


def test_symbols_declared_and_exported(hip_lib):
    # the entries' declarations, types and exports and header == ops for the constants: tests/test_abi_contract_cpu.py
    from pram_amd import _lib, ops
    header = (ROOT / "include" / "pram_hip.h").read_text()
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    for name, value in (("OBS_DOUBLES", IR.OBS_DOUBLES), ("GROUP_PARAMS", IR.NK), ("CONTEXT_BYTES", 1024)):
        assert value == getattr(ops, "BAC_" + name), name
    assert int(re.search(r"#define PRAM_BAC_ARRAYS (\d+)", header).group(1)) == len(ops.BAC_ARRAYS)
    assert [a[0] for a in ops.BAC_ARRAYS[:len(ops.BA_ARRAYS)]] == [a[0] for a in ops.BA_ARRAYS] and ops.CAMERA_NUM_PARAMS == IR.N_PARAMS
    # the existing entries keep their constants
    assert ops.BA_OBS_DOUBLES == 20 and int(re.search(r"#define PRAM_BA_ARRAYS (\d+)", header).group(1)) == 25
    src = (ROOT / "pram_amd" / "csrc" / "bundle.hip").read_text()
    assert not re.search(r"atomicAdd\(\s*(&\s*)?g\.(sd|J|x|r|z|p|q|k|kc|gx|gr|gz|gpv|gq|fpart|mvpart)\b", src)      # no floating-point atomics


def test_group_fold_runs_in_the_stated_order():
    x = np.arange(130, dtype=np.float64)[:, None] * np.array([1.0, 0.1])
    frames = np.arange(129, -1, -1)      # the order is the list's, not the frames'
    want = (x[frames[:64]].sum(0) + x[frames[64:128]].sum(0)) + x[frames[128:]].sum(0)
    assert np.array_equal(IR.group_fold(x, frames), want) and np.array_equal(IR.group_fold(x, frames[:1]), x[129])
    assert not IR.group_fold(x, frames[:0]).any()


# ---------------------------------------------------------------- J_k
def test_parameter_jacobians_agree_with_central_differences():
    """Every model.  The residual is linear in every intrinsic parameter (focal lengths, principal point and all four distortion
    coefficients enter fx ud + cx linearly), so a central difference has no truncation error and the step only sets the rounding,
    1e-16 |r| / h: h = 1e-2 max(|parameter|, 1)."""
    c = IR.gpu_case("models_pp")
    gp = c["problem"]
    pr = gp.pr
    J, ok, ex = IR.linearise(gp, pr.table, pr.xyz, gp.k0)
    rng = np.random.RandomState(1)
    worst = {}
    for q in range(gp.G):
        obs = np.nonzero(ok & (gp.frm_grp[pr.obs_frame] == q))[0]
        obs = rng.choice(obs, size=min(30, len(obs)), replace=False)
        n = IR.N_PARAMS[gp.model[q]]
        assert not ex["Jk"][obs][:, :, n:].any()      # zero padded
        for a in range(n):
            h = 1e-2 * max(abs(gp.k0[q, a]), 1.0)

            def res(d):
                k = gp.k0.copy()
                k[q, a] += d
                gp.set_cameras(k)
                _, r0, r1 = pr.residual(pr.table, pr.xyz)
                return np.stack([r0[obs], r1[obs]], 1)
            num = (res(h) - res(-h)) / (2 * h)
            scale = np.abs(ex["Jk"][obs]).max(axis=(1, 2))
            worst[gp.model[q]] = max(worst.get(gp.model[q], 0.0), float((np.abs(num - ex["Jk"][obs][:, :, a]).max(1) / scale).max()))
    gp.set_cameras(gp.k0)
    print("central differences of J_k, relative to the largest entry, per model: " + ", ".join(f"{m}: {e:.2e}" for m, e in sorted(worst.items())))
    assert sorted(worst) == [0, 1, 2, 3, 4] and max(worst.values()) < 5e-10
    # the weights and the frozen columns
    fz = gp.frozen_bits()[gp.frm_grp[pr.obs_frame]]
    for i in range(2):
        blk = J[:, 12 + 8 * i:20 + 8 * i]
        assert not blk[fz].any() and np.allclose(blk[ok], np.where(fz, 0.0, ex["sw"][:, None] * ex["Jk"][:, i])[ok], rtol=1e-15)
    assert not J[~ok].any()


# ---------------------------------------------------------------- the reduced system
@pytest.fixture(scope="module")
def system():
    c = IR.gpu_case("models_pp")
    gp = c["problem"]
    pr = gp.pr
    lam = 1e-3
    J, ok, _ = IR.linearise(gp, pr.table, pr.xyz, gp.k0)
    J20 = J[:, IR._J20]
    Vinv, g_p, good = BR.point_blocks(pr, J20, ok, lam)
    S, dU, b = BR.frame_blocks(pr, J20, Vinv, g_p, lam)
    Sg, dUg, bg, part = IR.group_blocks(gp, J, Vinv, g_p, lam)
    return c, gp, lam, J, ok, Vinv, g_p, good, S, dU, b, Sg, dUg, bg


def test_three_pass_matvec_against_the_dense_reduced_matrix(system):
    c, gp, lam, J, ok, Vinv, g_p, good, S, dU, b, Sg, dUg, bg = system
    pr = gp.pr
    Sd = IR.reduced_dense(gp, J, Vinv, lam)
    rng = np.random.RandomState(2)
    v, vg = rng.normal(size=(pr.F, 6)), rng.normal(size=(gp.G, 8))
    q, qg = IR.matvec(gp, J, Vinv, dU, dUg, lam, v, vg)
    want = Sd @ np.concatenate([v.reshape(-1), vg.reshape(-1)])
    dev = np.abs(np.concatenate([q.reshape(-1), qg.reshape(-1)]) - want).max() / np.abs(want).max()
    # the frames' blocks are S's diagonal blocks.  A group's block is U_k + lam diag U_k - sum over its observations of W V^-1 W^T:
    # S's block plus the cross terms of two frames of the group that see one point, which the preconditioner leaves out
    blk = max(np.abs(BR._sym6(S[f]) - Sd[6 * f:6 * f + 6, 6 * f:6 * f + 6]).max() / np.abs(Sd[6 * f:6 * f + 6, 6 * f:6 * f + 6]).max() for f in range(pr.F))
    og, gblk, definite = gp.frm_grp[pr.obs_frame], [], []
    for g in range(gp.G):
        a = 6 * pr.F + 8 * g
        cross = np.zeros((8, 8))
        for p in range(pr.P):
            o = pr.pt_obs[pr.pt_off[p]:pr.pt_off[p + 1]]
            o = o[og[o] == g]
            W = [J[i, 12:28].reshape(2, 8).T @ J[i, 28:34].reshape(2, 3) for i in o.tolist()]
            v = Vinv[p]
            V = np.array([[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]])
            if W:
                cross += sum(W) @ V @ sum(W).T - sum(w @ V @ w.T for w in W)
        want_g = Sd[a:a + 8, a:a + 8] + cross
        gblk.append(float(np.abs(IR._sym8(Sg[g]) - want_g).max() / np.abs(want_g).max()))
        definite.append(float(np.linalg.eigvalsh(IR._sym8(Sg[g])).min()))
    print(f"matvec against the dense reduced matrix {dev:.2e}; frame blocks {blk:.2e}; group blocks {max(gblk):.2e}, their smallest eigenvalue {min(definite):.2e}")
    assert dev < 1e-12 and blk < 1e-12 and max(gblk) < 1e-12 and min(definite) > 0.0
    assert np.allclose(Sd, Sd.T, rtol=0, atol=1e-9 * np.abs(Sd).max()) and np.linalg.eigvalsh(Sd).min() > 0.0


def test_pcg_against_dense_solves(system):
    """PCG run to a residual of 1e-13 |b| against numpy.linalg.solve on the dense reduced matrix and against the camera and
    intrinsics part of the full normal equations' solution, at tests/test_bundle_cpu.py's bars for the same two comparisons (1e-8
    and 1e-6).  Measured: 3.2e-11 against the solve, 3.2e-11 and 5.8e-11 against the full normal equations, in 120 iterations at
    cond(S) = 9.3e7, whose product with the rounding, 1e-8, is what either solve can promise."""
    c, gp, lam, J, ok, Vinv, g_p, good, S, dU, b, Sg, dUg, bg = system
    pr = gp.pr
    Sd = IR.reduced_dense(gp, J, Vinv, lam)
    x, xg, n, tr = IR.pcg(gp, J, Vinv, S, Sg, dU, dUg, b, bg, lam, 2000, 1e-13)
    got = np.concatenate([x.reshape(-1), xg.reshape(-1)])
    xs = np.linalg.solve(Sd, np.concatenate([b.reshape(-1), bg.reshape(-1)]))
    d, _, _ = IR.dense_step(gp, pr.table, pr.xyz, gp.k0, lam)
    nc = 6 * pr.F + 8 * gp.G
    _, acc = IR.mv_points(gp, J, Vinv, x, xg)
    dp = -BR._vinv_mul(Vinv, g_p + acc)
    solv = np.repeat(good, 3)
    cond = np.linalg.cond(Sd)
    e_s, e_c = np.abs(got - xs).max() / np.abs(xs).max(), np.abs(got - d[:nc]).max() / np.abs(d[:nc]).max()
    e_p = np.abs(dp.reshape(-1) - d[nc:])[solv].max() / np.abs(d[nc:]).max()
    print(f"PCG ({n} iterations, cond(S) {cond:.1e}) against numpy.linalg.solve on S {e_s:.2e}, against the full normal equations: "
          f"poses and intrinsics {e_c:.2e}, points {e_p:.2e}")
    assert e_s < PCG_SOLVE_BAR and e_c < PCG_FULL_BAR and e_p < PCG_FULL_BAR
    # steps of frozen and absent parameters: exactly 0
    fz = gp.frozen_bits()
    assert not xg[fz].any() and xg[~fz].all() and not x[pr.fmask == 63].any() and not x[pr.fmask == 8][:, 3].any()
    assert fz[4, 6] and not fz[4, 7] and fz[0, 3:].all() and not fz[0, :3].any()      # the per-group mask; SIMPLE_PINHOLE's absent five


PCG_SOLVE_BAR, PCG_FULL_BAR = 1e-8, 1e-6      # tests/test_bundle_cpu.py's bars for the same two comparisons


def test_every_intrinsic_frozen_is_bundle_ref_bit_for_bit():
    c = IR.gpu_case("models")
    gp, _ = IR.group_problem(c["scene"], c["model"], c["frozen"], c["frm_grp"], (False, False, False))
    assert (gp.gmask == 255).all()
    a, b = IR.run(gp, max_iters=5), BR.run(BR.gpu_case("special")["problem"], max_iters=5)
    assert np.array_equal(a["table"], b["table"]) and np.array_equal(a["xyz"], b["xyz"]) and a["final_cost"] == b["final_cost"]
    assert a["accepted"].tolist() == b["accepted"].tolist() and a["cg_iterations"].tolist() == b["cg_iterations"].tolist()
    assert np.array_equal(a["params"], gp.k0)
    # a candidate with a focal length at or below 0 is rejected as a NaN cost is
    k = gp.k0.copy()
    kc, bad = IR.candidate_params(gp, k, np.where(np.arange(8)[None] == 0, -2.0 * k, 0.0))
    assert bad and not IR.candidate_params(gp, k, np.zeros_like(k))[1] and np.array_equal(IR.candidate_params(gp, k, np.zeros_like(k))[0], k)


# ---------------------------------------------------------------- recovery on the planted scene
def _errors(c, r):
    truth, gp = c["truth"], c["problem"]
    kt = np.stack([np.pad(np.asarray(truth["cameras"][int(np.nonzero(c["frm_grp"] == q)[0][0])][3], dtype=np.float64), (0, 8))[:8] for q in range(gp.G)])
    rot, cen = BR.pose_errors(r["table"], truth["table"])
    return float(np.abs(r["params"][:, 0] / kt[:, 0] - 1.0).max()), float(np.abs(r["params"][:, 3] - kt[:, 3]).max()), float(rot.max()), float(cen.max())


def _recovery(noise, outliers):
    c = dict(IR.recovery_case(noise=noise, outliers=outliers))
    c["problem"], c["tables"] = IR.group_problem(c["scene"], c["model"], c["frozen"], c["frm_grp"], (True, False, True))
    return c


@pytest.fixture(scope="module")
def clean():
    c = _recovery(0.0, 0.0)
    p = dict(max_iters=40, ftol=1e-12, cg_iters=300, cg_tol=1e-6)
    return c, IR.run(c["problem"], **p), IR.dense_run(c["problem"], **p)


def test_recovery_without_noise(clean):
    """Measured (12 frames, 2 groups, 120 points, ftol 1e-12): the dense form ends at a focal error of 1.90e-8 relative, a k1 error
    of 1.21e-7 and 1.98e-6 degrees, and the sparse form at the same three figures (both stop on ftol at a cost of 8.8e-8, where
    the float32 keypoints bound what can be recovered).  The bar on the sparse form is ten times the dense form's figure of the
    same run."""
    c, r, d = clean
    e0 = _errors(c, {"params": c["problem"].k0, "table": c["problem"].pr.table})
    er, ed = _errors(c, r), _errors(c, d)
    print(f"start: focal {e0[0]:.2e}, k1 {e0[1]:.2e}, rotation {e0[2]:.2e} degrees; sparse: focal {er[0]:.2e}, k1 {er[1]:.2e}, rotation {er[2]:.2e} "
          f"(cost {r['final_cost']:.2e}, {len(r['accepted'])} iterations, CG {r['cg_iterations'].tolist()}); dense: focal {ed[0]:.2e}, k1 {ed[1]:.2e}, "
          f"rotation {ed[2]:.2e} (cost {d['final_cost']:.2e}, {d['iterations']} iterations)")
    assert e0[0] > 0.049 and e0[1] > 0.049
    assert er[0] <= 10 * ed[0] and er[1] <= 10 * ed[1] and er[2] <= 10 * ed[2]
    assert ed[0] < 1e-6 and ed[1] < 1e-6 and ed[2] < 1e-4      # the dense form does recover the planted camera


@pytest.fixture(scope="module")
def noisy():
    c = _recovery(0.5, 0.03)
    p = dict(max_iters=40, ftol=1e-12, cg_iters=300, cg_tol=1e-6)
    return c, IR.run(c["problem"], **p), IR.dense_run(c["problem"], **p)


def test_recovery_with_noise_and_outliers(noisy):
    """0.5 px noise, 3 % gross outliers: the bar is the dense form's result on the same data, not the planted values.  Both forms
    minimise the same cost; they are compared at their optima."""
    c, r, d = noisy
    gp = c["problem"]
    er, ed = _errors(c, r), _errors(c, d)
    lin = np.abs(r["params"] - d["params"])
    rot, cen = BR.pose_errors(r["table"], d["table"])
    print(f"sparse against dense: focal {np.abs(r['params'][:, 0] / d['params'][:, 0] - 1).max():.2e} relative, k1 {lin[:, 3].max():.2e}, rotation "
          f"{rot.max():.2e} degrees, centres {cen.max():.2e}, cost {r['final_cost']:.6f} / {d['final_cost']:.6f}; distance to the planted values: sparse "
          f"focal {er[0]:.2e}, k1 {er[1]:.2e}, rotation {er[2]:.2e} degrees; dense focal {ed[0]:.2e}, k1 {ed[1]:.2e}, rotation {ed[2]:.2e}")
    assert abs(r["final_cost"] - d["final_cost"]) <= 1e-9 * d["final_cost"]
    assert np.abs(r["params"][:, 0] / d["params"][:, 0] - 1).max() < 1e-6 and lin[:, 3].max() < 1e-6 and rot.max() < 1e-4 and cen.max() < 1e-5
    assert er[0] < 0.01 and er[1] < 0.02      # and it is a recovery: from 5 % and 0.05


def test_constant_intrinsics_end_worse(noisy):
    """The control: the same data with the flags off ends at a visibly higher cost and a larger pose error."""
    c, r, _ = noisy
    gp0, _ = IR.group_problem(c["scene"], c["model"], c["frozen"], c["frm_grp"], (False, False, False))
    off = IR.run(gp0, max_iters=40, ftol=1e-12, cg_iters=300, cg_tol=1e-6)
    e_on, e_off = _errors(c, r), _errors(c, off)
    print(f"flags off: cost {off['final_cost']:.1f}, rotation {e_off[2]:.3f} degrees, centres {e_off[3]:.3f}; flags on: cost {r['final_cost']:.1f}, "
          f"rotation {e_on[2]:.3f} degrees, centres {e_on[3]:.3f}")
    assert off["final_cost"] > r["final_cost"] and e_off[2] > e_on[2] and e_off[3] > e_on[3]


def test_stationarity_against_scipy(noisy):
    """scipy.optimize.least_squares (trf, 2-point Jacobian with the sparsity pattern) on the same robust cost over poses, free
    intrinsics and points, from the restatement's optimum.  Measured: the cost falls by 1.94e-15 relative, the focal lengths move by
    5.28e-11 relative and the poses by 1.25e-9 degrees (12 frames, 2 groups, 120 points, 3 % outliers); the bars are ten times that."""
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix
    c, r, _ = noisy
    gp = c["problem"]
    pr = gp.pr
    free = np.nonzero(pr.fmask != 63)[0]
    fz = gp.frozen_bits()
    kfree = [(q, a) for q in range(gp.G) for a in range(8) if not fz[q, a]]
    table0, xyz0, k0 = r["table"], r["xyz"], r["params"]
    n_c, n_k = 6 * len(free), len(kfree)

    def unpack(v):
        table, k = table0.copy(), k0.copy()
        for i, f in enumerate(free.tolist()):
            table[f] = BR.rodrigues_update(table0[f], v[6 * i:6 * i + 6])
        for i, (q, a) in enumerate(kfree):
            k[q, a] = k0[q, a] + v[n_c + i] * SCALE[a]
        return table, k, xyz0 + v[n_c + n_k:].reshape(-1, 3)

    SCALE = np.array([500.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])      # a focal length in units of 500 px, so that one step serves all

    def fun(v):
        table, k, xyz = unpack(v)
        gp.set_cameras(k)
        _, r0, r1 = pr.residual(table, xyz)
        sq = r0 * r0 + r1 * r1
        g = np.sqrt(np.where(sq > 0, np.log1p(sq) / np.where(sq > 0, sq, 1.0), 1.0))
        return np.stack([g * r0, g * r1], 1).reshape(-1)

    n = n_c + n_k + 3 * pr.P
    pat = lil_matrix((2 * pr.O, n), dtype=int)
    col = {f: i for i, f in enumerate(free.tolist())}
    for o in range(pr.O):
        f, p = int(pr.obs_frame[o]), int(pr.obs_point[o])
        if f in col:
            pat[2 * o:2 * o + 2, 6 * col[f]:6 * col[f] + 6] = 1
        for i, (q, a) in enumerate(kfree):
            if q == gp.frm_grp[f]:
                pat[2 * o:2 * o + 2, n_c + i] = 1
        pat[2 * o:2 * o + 2, n_c + n_k + 3 * p:n_c + n_k + 3 * p + 3] = 1
    c0 = float((fun(np.zeros(n)) ** 2).sum())
    assert abs(c0 - r["final_cost"]) <= 1e-9 * c0      # the same cost
    sol = least_squares(fun, np.zeros(n), jac_sparsity=pat, method="trf", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=30)
    c1 = float((sol.fun ** 2).sum())
    table1, k1, _ = unpack(sol.x)
    gp.set_cameras(gp.k0)
    rot, _ = BR.pose_errors(table1, table0)
    df = float(np.abs(k1[:, 0] / k0[:, 0] - 1).max())
    print(f"scipy: cost {c0:.9f} -> {c1:.9f} (relative {(c0 - c1) / c0:.2e}), focal lengths moved by {df:.2e} relative, poses by {rot.max():.2e} degrees")
    assert (c0 - c1) / c0 <= STATIONARY_COST and df <= STATIONARY_FOCAL and rot.max() <= STATIONARY_ROT


STATIONARY_COST, STATIONARY_FOCAL, STATIONARY_ROT = 1.95e-14, 5.3e-10, 1.3e-8      # ten times the measured values (the docstring above)


# ---------------------------------------------------------------- the margins of every run the GPU test makes
@pytest.mark.parametrize("name", sorted(IR.GPU_RUNS))
def test_margins_the_gpu_test_relies_on(name):
    c, r = IR.gpu_case(name), IR.gpu_run(name)
    gp = c["problem"]
    pr = gp.pr
    m, flt, p = r["margins"], r["filter"], {**BR.DEFAULTS, **c["params"]}
    print(f"{name}: {gp.G} groups of {np.diff(gp.grp_off).tolist()} frames, masks {gp.gmask.tolist()}; {len(r['accepted'])} iterations, accepted "
          f"{r['accepted'].astype(int).tolist()}, CG {r['cg_iterations'].tolist()}, {r['termination']}; accept margin {m['accept'].min():.2e}, CG stop margin "
          f"{m['cg'].min():.2e}; cost {r['initial_cost']:.1f} -> {r['final_cost']:.1f}")
    assert (m["accept"] > 1e-9).all() and (m["cg"] > 1e-9).all() and r["cg_breakdowns"] == 0
    assert len(r["accepted"]) == p["max_iters"] or r["termination"] == "ftol"
    assert r["accepted"].any() and r["final_cost"] < r["initial_cost"]
    err, ang = flt["obs_error"][np.isfinite(flt["obs_error"])], flt["pt_angle"][flt["pt_angle"] >= 0]
    assert (np.abs(err - p["max_reproj_error"]) > 1e-6).all() and (np.abs(ang - np.deg2rad(p["min_tri_angle"])) > 1e-9).all()
    fz = gp.frozen_bits()
    assert np.array_equal(r["params"][fz], gp.k0[fz]) and (r["params"][~fz] != gp.k0[~fz]).all()
    foc = np.concatenate([r["params"][q, list(IR.FOCAL[gp.model[q]])] for q in range(gp.G)])
    assert (foc > 100.0).all()      # no candidate near the focal test
    if name.startswith("models"):
        assert sorted(gp.model.tolist()) == [0, 1, 2, 3, 4] and [IR.N_PARAMS[i] for i in gp.model] == [3, 4, 4, 5, 8]
        assert np.diff(gp.frames_of(0)).tolist() == [5, 5] and np.diff(pr.frm_off)[11] == 0
        assert (name == "models_pp") == (not fz[1, 2]) and (name == "models_pp") == bool(fz[4, 6] and not fz[4, 7])
    if name == "ring":
        assert r["accepted"].tolist() == [True, True, False, True]      # a rejected step, and the accepted one after it
        assert gp.G == 1 and len(gp.frames_of(0)) == 70 > BR.BLOCK and sorted(np.diff(pr.pt_off).tolist())[-1] == 65 and (pr.fmask[30:] == 63).all()
    if name == "frames":
        assert np.diff(pr.frm_off).tolist()[:6] == [0, 1, 63, 64, 65, 257] and np.diff(gp.grp_off).tolist() == [2, 2, 1, 1, 1]
        assert (pr.fmask[gp.frames_of(0)] == 63).all() and (pr.fmask[gp.frames_of(1)] == [0, 63]).all() and gp.gmask[0] != 255
    if name == "split":
        assert gp.frames_of(0).tolist() == [0, 2, 4, 6] and gp.frames_of(1).tolist() == [1, 3, 5, 7] and gp.frames_of(2).tolist() == [8]
        assert pr.fmask[8] == 63 and gp.n_obs[3] == 0 and gp.gmask[3] == 255 and gp.mask_in[3] != 255 and np.array_equal(r["params"][3], gp.k0[3])


# ---------------------------------------------------------------- the host side, ops replaced by the restatement
def _stub_class():
    from tests.test_bundle_cpu import StubOps

    class StubCamOps(StubOps):
        """StubOps with the pram_bac_* calls, computed by bundle_intr_ref."""

        def __init__(self):
            super().__init__()
            from pram_amd import ops
            for k in ("CAMERA_NUM_PARAMS", "CAMERA_MODELS"):
                setattr(self, k, getattr(ops, k))

        def bac_begin(self, keypoints, cam_model, cam_model_host, table, xyz, obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen, frm_grp,
                      grp_off, grp_frame, grp_params, grp_mask, n_points, n_obs, n_rows, n_groups, max_iters, **kw):
            self.calls.append("bac_begin")
            F, G = len(cam_model_host), n_groups
            g = frm_grp.numpy()[:F]
            prm = grp_params.numpy()[:G]
            prob = self.ba_begin(keypoints, cam_model, torch.from_numpy(prm[g].copy()), cam_model_host, table, xyz, obs_row, obs_frame, obs_point,
                                 frm_off, pt_off, pt_obs, frozen, n_points, n_obs, n_rows, max_iters, **kw)
            self.calls.pop()
            gp = IR.GroupProblem(prob["problem"], g, prm, grp_mask.numpy()[:G])
            assert np.array_equal(gp.grp_off, grp_off.numpy()[:G + 1]) and np.array_equal(gp.grp_frame, grp_frame.numpy()[:F])
            return {**prob, "group_problem": gp, "n_groups": G}

        def bac_iterate(self, prob, n_iters, cg_iters, stages=31):
            self.calls.append("bac_iterate")
            if prob["result"] is not None:
                return
            real, BR.run = BR.run, lambda pr, **kw: IR.run(prob["group_problem"], **kw)
            try:
                self.ba_iterate(prob, n_iters, cg_iters, stages)
            finally:
                BR.run = real
            self.calls.pop()

        def bac_finish(self, prob, qvec, tvec, **kw):
            self.calls.append("bac_finish")
            gp = prob["group_problem"]
            r = prob["result"] or IR.run(gp, **{**prob["params"], "max_iters": 0})
            prob["result"] = r
            gp.set_cameras(r["params"])
            out = self.ba_finish(prob, qvec, tvec, **kw)
            self.calls.pop()
            return {**out, "grp_params": torch.from_numpy(r["params"].copy())}
    return StubCamOps


@pytest.fixture()
def stubbed(monkeypatch):
    from pram_amd.localization import bundle as BA
    from pram_amd.localization import triangulation as TG
    stub = _stub_class()()
    monkeypatch.setattr(TG, "ops", stub)
    monkeypatch.setattr(BA, "ops", stub)
    monkeypatch.setattr(TG, "_device", lambda device: torch.device("cpu"))
    return BA, stub


def _args(c):
    s = c["scene"]
    return s["frames"], s["cameras"], (s["qvec"], s["tvec"]), c["model"]


def test_host_logic_with_ops_stubbed(stubbed):
    BA, stub = stubbed
    c, r = IR.gpu_case("models"), IR.gpu_run("models")
    gp = c["problem"]
    # ---- the default grouping: equal tuples share a group, numbered by first appearance
    cams = c["scene"]["cameras"]
    assert BA.camera_groups(cams).tolist() == (np.arange(12) % 5).tolist() and BA.camera_groups(cams).dtype == np.int32
    assert BA.camera_groups(cams, np.arange(12) % 5 + 7).tolist() == (np.arange(12) % 5).tolist()      # an explicit grouping, renumbered
    assert BA.camera_groups(cams, np.arange(12)).tolist() == list(range(12))                            # finer than the cameras: allowed
    near = list(cams)
    near[5] = (cams[5][0], cams[5][1], cams[5][2], [515.0 + 1e-13, 320.5, 239.0])
    assert BA.camera_groups(near)[5] == 5 and BA.camera_groups(near).max() == 5                         # bit-equal parameters only
    # ---- a flag on: the new entries, the restatement's numbers
    m = BA.bundle_adjust(*_args(c), "cpu", frozen=c["frozen"], refine_focal_length=True, refine_extra_params=True, **c["params"])
    assert stub.calls[0] == "bac_begin" and stub.calls[-1] == "bac_finish" and "ba_begin" not in stub.calls
    rep = m["report"]
    assert rep["accepted"].tolist() == r["accepted"].tolist() and rep["final_cost"] == r["final_cost"] and rep["termination"] == r["termination"]
    assert np.array_equal(m["camera_groups"], c["frm_grp"]) and len(m["cameras"]) == 12 and len(rep["intrinsics"]) == 5
    for q, row in enumerate(rep["intrinsics"]):
        n = IR.N_PARAMS[gp.model[q]]
        assert row["model"] == cams[q][0] and row["frames"] == len(gp.frames_of(q)) and row["observations"] == gp.n_obs[q] and row["mask"] == gp.gmask[q]
        assert np.array_equal(row["params_before"], gp.k0[q, :n]) and np.array_equal(row["params_after"], r["params"][q, :n])
    for f, cam in enumerate(m["cameras"]):
        q = int(c["frm_grp"][f])
        assert cam[:3] == tuple(cams[f][:3]) and np.array_equal(cam[3], r["params"][q, :IR.N_PARAMS[gp.model[q]]])
    # ---- the flags select the masks
    p = BA._ba_params("t", dict(refine_principal_point=True))
    assert BA.group_tables(cams, BA.camera_groups(cams), p)["grp_mask"].tolist() == [255 & ~0b110, 255 & ~0b1100, 255 & ~0b110, 255 & ~0b110, 255 & ~0b1100]
    p = BA._ba_params("t", dict(refine_focal_length=True, refine_extra_params=True))
    assert BA.group_tables(cams, BA.camera_groups(cams), p)["grp_mask"].tolist() == gp.mask_in.tolist()
    # ---- all flags False: the existing path, with and without camera_groups; the cameras come back as they are
    stub.calls.clear()
    z = BA.bundle_adjust(*_args(c), "cpu", frozen=c["frozen"], max_iters=2, camera_groups=np.arange(12) % 5)
    assert stub.calls[0] == "ba_begin" and not any(k.startswith("bac_") for k in stub.calls)
    assert all(a is b for a, b in zip(z["cameras"], cams)) and z["report"]["intrinsics"] == [] and z["camera_groups"].tolist() == (np.arange(12) % 5).tolist()
    # ---- a group without observations is frozen: its frames get their input tuples back
    s = IR.gpu_case("split")
    ms = BA.bundle_adjust(*_args(s), "cpu", frozen=s["frozen"], max_iters=3, camera_groups=s["frm_grp"], refine_focal_length=True)
    rows = ms["report"]["intrinsics"]
    assert rows[3]["mask"] == 255 and rows[3]["observations"] == 0 and ms["cameras"][9] is s["scene"]["cameras"][9]
    assert rows[0]["frames"] == 4 and not np.array_equal(rows[0]["params_after"], rows[0]["params_before"])
    # ---- refusals
    F = 12
    for bad in (dict(camera_groups=np.zeros(F, dtype=np.int64)), dict(camera_groups=np.zeros(F - 1, dtype=np.int64)), dict(camera_groups=np.zeros((F, 1), dtype=np.int64)),
                dict(camera_groups=np.arange(F) % 5 * 1.0), dict(camera_groups=-(np.arange(F) % 5)), dict(refine_focal_length=1), dict(refine_extra_params="yes"),
                dict(refine_principal_point=None)):
        for flag in ({}, {"refine_focal_length": True}):
            with pytest.raises(ValueError):
                BA.bundle_adjust(*_args(c), "cpu", **{**flag, **bad})
    with pytest.raises(TypeError):
        BA.bundle_adjust(*_args(c), "cpu", refine_focal=True)
    # ---- an empty model
    empty = {"point_ids": np.zeros(0, dtype=np.int64), "point3D_xyzs": np.zeros((0, 3)), "track_error": np.zeros(0), "tracks": {}, "point3D_frame_ids": {}}
    m0 = BA.bundle_adjust(*_args(c)[:3], empty, "cpu", refine_focal_length=True)
    assert m0["report"]["termination"] == "empty" and all(a is b for a, b in zip(m0["cameras"], cams)) and len(m0["report"]["intrinsics"]) == 5
    assert all(row["mask"] == 255 for row in m0["report"]["intrinsics"])


def test_mapper_passes_the_flags_to_the_final_adjustment_only(monkeypatch):
    """reconstruct's bundle= dict: _map_params takes the flags, _adjust (the per-round solve) reads none of them and calls the
    entries with constant intrinsics, the final bundle_adjust receives them."""
    import inspect
    from pram_amd.localization import bundle as BA
    from pram_amd.localization import mapper as MP
    p = MP._map_params("t", dict(bundle=dict(refine_focal_length=True, camera_groups=np.zeros(3, dtype=np.int64))))
    assert p["bundle"]["refine_focal_length"] is True and p["bundle"]["refine_extra_params"] is False
    with pytest.raises(ValueError):
        MP._map_params("t", dict(bundle=dict(refine_focal_length="yes")))
    src = inspect.getsource(MP._adjust)
    assert "ops.ba_begin(" in src and "bac_" not in src and "refine_" not in src and "camera_groups" not in src
    seen = {}

    def fake(frames, cameras, poses, model, device, **kw):
        seen.update(kw)
        raise RuntimeError("reached")
    monkeypatch.setattr(BA, "bundle_adjust", fake)
    ba = {k: x for k, x in p["bundle"].items() if k not in MP._BA_OWN}
    with pytest.raises(RuntimeError):
        MP.bundle.bundle_adjust([], [], None, {}, "cpu", max_iters=1, frozen=None, **ba)
    assert seen["refine_focal_length"] is True and seen["refine_principal_point"] is False and "camera_groups" in seen
    assert "result['cameras']" in MP.reconstruct.__doc__ and "refine_focal_length" in MP.reconstruct.__doc__
