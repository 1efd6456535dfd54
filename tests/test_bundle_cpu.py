"""CPU: the numpy restatement of the bundle adjustment (tests/bundle_ref.py) against central differences, the dense reduced
matrix, a dense solve of the full normal equations and scipy; what it recovers on planted scenes; the margins that make the
discrete decisions of the GPU test's runs exact; and the host side of pram_amd.localization.bundle with ops replaced by the
restatement."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import bundle_ref as BR
from tests import pose_ref as PR
from tests import triangulation_ref as TR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_ba_workspace_bytes", "pram_ba_layout", "pram_ba_begin", "pram_ba_iterate", "pram_ba_finish")


def test_symbols_declared_and_exported(hip_lib):
    """The entries' declarations, types and exports and header == ops for the constants: tests/test_abi_contract_cpu.py."""
    from pram_amd import _lib, ops
    from pram_amd.localization import bundle as BA
    header = (ROOT / "include" / "pram_hip.h").read_text()
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    for name, value in (("OBS_DOUBLES", BR.OBS_DOUBLES), ("BLOCK", BR.BLOCK), ("CONTEXT_BYTES", 512), ("STATE_F64", 16), ("STATE_I32", 16),
                        ("SD_COST", 0), ("SD_LAM", 2), ("SD_COST0", 9), ("SI_DONE", 0), ("SI_REASON", 1), ("SI_LM_ITER", 2), ("SI_ACCEPTED", 3),
                        ("SI_CG_FAIL", 9), ("STAGE_ALL", 31)):
        assert value == getattr(ops, "BA_" + name), name
    assert int(re.search(r"#define PRAM_BA_ARRAYS (\d+)", header).group(1)) == len(ops.BA_ARRAYS)
    tri_src, obs_h = (ROOT / "pram_amd" / "csrc" / "triangulate.hip").read_text(), (ROOT / "pram_amd" / "csrc" / "obs.h").read_text()
    pose_src, ransac_h = (ROOT / "pram_amd" / "csrc" / "pose.hip").read_text(), (ROOT / "pram_amd" / "csrc" / "ransac.h").read_text()
    for helper in ("void obs_residual(", "bool chol_solve3(", "struct Obs"):      # shared, not restated
        assert helper in obs_h and helper not in tri_src, helper
    assert "void pose_update(" in ransac_h and "void pose_update(" not in pose_src
    bundle_src = (ROOT / "pram_amd" / "csrc" / "bundle.hip").read_text()
    assert "atomicAdd(counts" in bundle_src and not re.search(r"atomicAdd\(\s*(&\s*)?g\.(sd|J|x|r|z|p|q)\b", bundle_src)      # integer counters only
    assert BA.BA_DEFAULTS["lam0"] == PR.LM_LAMBDA0 and all(BA.BA_DEFAULTS[k] == v for k, v in BR.DEFAULTS.items())
    for word in ("Triggs", "Retriangulate", "pycolmap", "intrinsics", "gauge"):
        assert word in BA.__doc__, word


def test_sums_run_in_the_stated_orders():
    rng = np.random.RandomState(0)
    for n in (1, 63, 64, 65, 256, 257, 600):
        x = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-6, 6, size=(n, 1))
        assert np.allclose(BR.frame_sum(x), x.sum(0), rtol=1e-9, atol=1e-6)
        assert np.isclose(BR.blocked_sum(x[:, 0]), x[:, 0].sum(), rtol=1e-9, atol=1e-6)
    x = rng.normal(size=64)
    assert BR.frame_sum(x) == TR.wave_sum(x)      # fewer than 65 entries: the first wave's butterfly, three zeros folded in
    x = np.arange(130, dtype=np.float64)
    assert BR.blocked_sum(x) == (x[:64].sum() + x[64:128].sum()) + x[128:].sum()


@pytest.fixture(scope="module")
def special():
    c = BR.gpu_case("special")
    pr = c["problem"]
    J, ok, aux = BR.linearise(pr, pr.table, pr.xyz)
    return c, pr, J, ok, aux


def test_jacobians_agree_with_central_differences(special):
    c, pr, J, ok, aux = special
    rng = np.random.RandomState(1)
    h = 1e-6
    worst_c, worst_p = 0.0, 0.0
    for o in rng.choice(np.nonzero(ok)[0], size=40, replace=False).tolist():
        f, p = pr.obs_frame[o], pr.obs_point[o]

        def res(d, dx):
            table, xyz = pr.table.copy(), pr.xyz.copy()
            table[f] = BR.rodrigues_update(pr.table[f], d)
            xyz[p] = pr.xyz[p] + dx
            _, r0, r1 = pr.residual(table, xyz)
            return np.array([r0[o], r1[o]])

        for a in range(6):
            d = np.zeros(6); d[a] = h
            num = (res(d, np.zeros(3)) - res(-d, np.zeros(3))) / (2 * h)
            worst_c = max(worst_c, np.abs(num - aux["Jc"][o][:, a]).max() / np.abs(aux["Jc"][o]).max())
        for k in range(3):
            dx = np.zeros(3); dx[k] = h
            num = (res(np.zeros(6), dx) - res(np.zeros(6), -dx)) / (2 * h)
            worst_p = max(worst_p, np.abs(num - aux["Jp"][o][:, k]).max() / np.abs(aux["Jp"][o]).max())
    print(f"central differences, h = {h}: pose Jacobian within {worst_c:.2e}, point Jacobian within {worst_p:.2e} (relative to the largest entry)")
    assert worst_c < 1e-6 and worst_p < 1e-6      # the truncation error of a central difference at h = 1e-6 plus its rounding, 1e-16 / h
    # the weights, the frozen columns and the observation behind its camera
    s = aux["s"][ok]
    assert np.allclose(J[ok, 18:20], aux["r"][ok] / np.sqrt(1.0 + s)[:, None], rtol=1e-14)
    assert not J[pr.fmask[pr.obs_frame] == 63, :12].any() and not J[pr.fmask[pr.obs_frame] == 8][:, [3, 9]].any()
    assert (~ok).sum() == 1 and not J[~ok].any() and aux["z"][~ok][0] < 0.0


def test_schur_matvec_and_pcg_against_dense_forms(special):
    c, pr, J, ok, aux = special
    lam = 1e-3
    Vinv, gp, good = BR.point_blocks(pr, J, ok, lam)
    S, dU, b = BR.frame_blocks(pr, J, Vinv, gp, lam)
    Sd = BR.reduced_dense(pr, J, Vinv, dU, lam)
    rng = np.random.RandomState(2)
    v = rng.normal(size=(pr.F, 6))
    q, want = BR.matvec(pr, J, Vinv, dU, lam, v), (Sd @ v.reshape(-1)).reshape(pr.F, 6)
    dev = np.abs(q - want).max() / np.abs(want).max()
    # the diagonal blocks the preconditioner factors are S's
    blk = max(np.abs(BR._sym6(S[f]) - Sd[6 * f:6 * f + 6, 6 * f:6 * f + 6]).max() / np.abs(Sd[6 * f:6 * f + 6, 6 * f:6 * f + 6]).max() for f in range(pr.F))
    x, n, tr = BR.pcg(pr, J, Vinv, S, dU, b, lam, 500, 1e-13)
    xs = np.linalg.solve(Sd, b.reshape(-1)).reshape(pr.F, 6)
    # the independent form: the camera part of the full normal equations' solution, the points moved by the back-substitution
    d, _, _ = BR.dense_step(pr, pr.table, pr.xyz, lam)
    solv = np.repeat(good, 3)
    _, acc = BR.mv_points(pr, J, Vinv, x)
    dp = -BR._vinv_mul(Vinv, gp + acc)
    e_s, e_c = np.abs(x - xs).max() / np.abs(xs).max(), np.abs(x.reshape(-1) - d[:6 * pr.F]).max() / np.abs(d[:6 * pr.F]).max()
    e_p = np.abs(dp.reshape(-1) - d[6 * pr.F:])[solv].max() / np.abs(d[6 * pr.F:]).max()
    print(f"matvec against the dense reduced matrix {dev:.2e}; diagonal blocks {blk:.2e}; PCG ({n} iterations) against numpy.linalg.solve on S {e_s:.2e}, "
          f"against the full normal equations: poses {e_c:.2e}, points {e_p:.2e}")
    assert dev < 1e-12 and blk < 1e-12      # the same sums in another order
    assert e_s < 1e-8 and e_c < 1e-6 and e_p < 1e-6      # cond(S) times the solve's residual; the point the solve cannot move differs by design
    assert int((~good).sum()) == 1      # the point with one weighted observation
    # a frozen parameter's step is exactly 0
    assert not x[pr.fmask == 63].any() and not x[pr.fmask == 8][:, 3].any() and x[pr.fmask == 8][:, [0, 1, 2, 4, 5]].all()
    r = BR.gpu_run("special")
    assert np.array_equal(r["table"][pr.fmask == 63], pr.table[pr.fmask == 63]) and np.array_equal(r["table"][pr.fmask == 8][:, 9], pr.table[pr.fmask == 8][:, 9])
    assert not r["moved"][pr.fmask == 63].any() and r["moved"][pr.fmask != 63].all()
    assert np.array_equal(r["xyz"][~r["solvable"]], pr.xyz[~r["solvable"]])      # the point that cannot move stays


# ---------------------------------------------------------------- recovery
def _recovery_case(noise: float, outliers: float, rot: float, centre: float, seed: int):
    s = TR.tri_scene(noise=noise)
    rng = np.random.RandomState(seed)
    planted = {}
    if outliers > 0:
        s = dict(s)
        kp = s["keypoints"].copy()
        obs = sorted(s["where"].items())
        for i in rng.choice(len(obs), size=int(round(outliers * len(obs))), replace=False).tolist():
            (f, p), k = obs[i]
            a = rng.uniform(0, 2 * np.pi)
            row = int(s["frame_off"][f]) + k
            kp[row] = kp[row] + rng.uniform(15.0, 30.0) * np.array([np.cos(a), np.sin(a)], dtype=np.float32)
            planted[row] = p
        s["keypoints"] = kp
        s["norm05"] = TR.normalize(kp, s["frame_off"], s["cam_model"], s["cam_params"], 0.5)
    q, t = BR.perturb_poses(s, rot, centre, seed=seed + 1, keep=(0, TR.N_ARC - 1))
    sp = BR.with_poses(s, q, t)
    model, which = BR.triangulated_model(sp, max_reproj_error=60.0)
    frozen = np.zeros(s["n_frames"], dtype=np.int64)
    frozen[[0, TR.N_ARC - 1]] = 63
    pr, tabs = BR.problem_of(sp, model, frozen=frozen)
    return s, sp, {**model, "planted": which}, pr, planted


def _pose_err(table, truth, pr):
    seen = np.diff(pr.frm_off) > 0
    rot, cen = BR.pose_errors(table, truth["table"])
    return float(rot[seen].max()), float(cen[seen].max())


@pytest.fixture(scope="module")
def noisy_case():
    s, sp, model, pr, planted = _recovery_case(0.5, 0.03, 2.0, 0.1, seed=21)
    return s, sp, model, pr, planted, BR.run(pr, ftol=1e-12, cg_tol=1e-6, max_iters=60), BR.dense_run(pr, ftol=1e-12, max_iters=60)


def test_recovery_without_noise():
    """Frames 0 and 9 frozen at their true poses, the others off by about 1 degree and 3 % of the baseline, the points from the
    restated triangulation with those poses.  Measured: the dense form comes back to 1.5e-6 degrees, 2.2e-7 in the centres
    and 6.3e-7 in the points (the keypoints are float32), the restatement to the same figures."""
    s, sp, model, pr, _ = _recovery_case(0.0, 0.0, 1.0, 0.3, seed=0)
    r, d = BR.run(pr), BR.dense_run(pr)
    ids = model["planted"]
    er, ed = _pose_err(r["table"], s, pr), _pose_err(d["table"], s, pr)
    pr_, pd_ = np.abs(r["xyz"] - s["xyz"][ids]).max(), np.abs(d["xyz"] - s["xyz"][ids]).max()
    print(f"before {_pose_err(sp['table'], s, pr)}; restatement {er}, points {pr_:.2e}, {len(r['accepted'])} iterations; dense {ed}, points {pd_:.2e}")
    assert _pose_err(sp["table"], s, pr)[0] > 0.5
    assert er[0] <= 10 * ed[0] and er[1] <= 10 * ed[1] and pr_ <= 10 * pd_ and ed[0] < 1e-4 and ed[1] < 1e-5


def test_recovery_with_noise_and_outliers(noisy_case):
    s, sp, model, pr, planted, r, d = noisy_case
    e0, er, ed = _pose_err(sp["table"], s, pr), _pose_err(r["table"], s, pr), _pose_err(d["table"], s, pr)
    flt = r["filter"]
    is_out = np.array([row in planted for row in pr.obs_row.tolist()])
    lost_true = int((~flt["obs_keep"] & ~is_out).sum())
    print(f"rotation {e0[0]:.3f} -> {er[0]:.3f} degrees (dense {ed[0]:.3f}), centre {e0[1]:.3f} -> {er[1]:.3f} (dense {ed[1]:.3f}); "
          f"{int(is_out.sum())} planted outliers in the model, {int((~flt['obs_keep'] & is_out).sum())} filtered; {lost_true} of {int((~is_out).sum())} true observations filtered")
    assert is_out.sum() >= 0.02 * pr.O
    assert er[0] / e0[0] <= 2 * ed[0] / e0[0] and er[1] / e0[1] <= 2 * ed[1] / e0[1] and ed[0] < 0.5 * e0[0]
    assert not flt["obs_keep"][is_out].any() and lost_true <= 0.02 * (~is_out).sum()


def test_stationarity_against_scipy(noisy_case):
    """scipy.optimize.least_squares (trf, 2-point Jacobian with the sparsity pattern) on the same cost, from the restatement's
    optimum (run to ftol = 1e-12 with cg_tol = 1e-6).  Measured: the cost falls by 4.3e-16 relative, the poses move by 3.8e-10
    degrees and 3.6e-11 (12 frames, 299 points, 1782 observations, 3 % outliers); the bars are ten times that."""
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix
    s, sp, model, pr, planted, r, d = noisy_case
    free = np.nonzero(pr.fmask != 63)[0]
    table0, xyz0 = r["table"], r["xyz"]

    def unpack(v):
        table = table0.copy()
        for i, f in enumerate(free.tolist()):
            table[f] = BR.rodrigues_update(table0[f], v[6 * i:6 * i + 6])
        return table, xyz0 + v[6 * len(free):].reshape(-1, 3)

    def fun(v):
        table, xyz = unpack(v)
        _, r0, r1 = pr.residual(table, xyz)
        sq = r0 * r0 + r1 * r1
        g = np.sqrt(np.where(sq > 0, np.log1p(sq) / np.where(sq > 0, sq, 1.0), 1.0))      # |g r|^2 = log1p(|r|^2)
        return np.stack([g * r0, g * r1], 1).reshape(-1)

    n = 6 * len(free) + 3 * pr.P
    pat = lil_matrix((2 * pr.O, n), dtype=int)
    col = {f: i for i, f in enumerate(free.tolist())}
    for o in range(pr.O):
        f, p = int(pr.obs_frame[o]), int(pr.obs_point[o])
        if f in col:
            pat[2 * o:2 * o + 2, 6 * col[f]:6 * col[f] + 6] = 1
        pat[2 * o:2 * o + 2, 6 * len(free) + 3 * p:6 * len(free) + 3 * p + 3] = 1
    c0 = float((fun(np.zeros(n)) ** 2).sum())
    assert abs(c0 - r["final_cost"]) <= 1e-9 * c0      # the same cost
    sol = least_squares(fun, np.zeros(n), jac_sparsity=pat, method="trf", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=30)
    c1 = float((sol.fun ** 2).sum())
    table1, _ = unpack(sol.x)
    rot, cen = BR.pose_errors(table1, table0)
    print(f"scipy: cost {c0:.9f} -> {c1:.9f} (relative {(c0 - c1) / c0:.2e}), poses moved by {rot.max():.2e} degrees and {cen.max():.2e}")
    assert (c0 - c1) / c0 <= STATIONARY_COST and rot.max() <= STATIONARY_ROT and cen.max() <= STATIONARY_CEN


STATIONARY_COST, STATIONARY_ROT, STATIONARY_CEN = 4.4e-15, 3.8e-9, 3.7e-10      # ten times the measured values (the docstring above)


# ---------------------------------------------------------------- the margins of every run the GPU test makes
@pytest.mark.parametrize("name", sorted(BR.GPU_RUNS))
def test_margins_the_gpu_test_relies_on(name):
    c, r = BR.gpu_case(name), BR.gpu_run(name)
    m, flt, p = r["margins"], r["filter"], {**BR.DEFAULTS, **c["params"]}
    print(f"{name}: {len(r['accepted'])} iterations, accepted {r['accepted'].astype(int).tolist()}, CG {r['cg_iterations'].tolist()}, {r['termination']}; "
          f"accept margin {m['accept'].min() if len(m['accept']) else np.inf:.2e}, CG stop margin {m['cg'].min() if len(m['cg']) else np.inf:.2e}")
    assert (m["accept"] > 1e-9).all() and (m["cg"] > 1e-9).all() and r["cg_breakdowns"] == 0
    assert len(r["accepted"]) == p["max_iters"] or r["termination"] == "ftol"
    err, ang = flt["obs_error"][np.isfinite(flt["obs_error"])], flt["pt_angle"][flt["pt_angle"] >= 0]
    assert (np.abs(err - p["max_reproj_error"]) > 1e-6).all() and (np.abs(ang - np.deg2rad(p["min_tri_angle"])) > 1e-9).all()
    z, _, _ = c["problem"].residual(r["table"], r["xyz"])
    assert (np.abs(z) > 1e-6).all()
    if name == "special":
        ids = c["model"]["point_ids"].tolist()
        behind, low = ids.index(c["behind"]), ids.index(c["low_angle"])
        assert not flt["pt_keep"][behind] and not flt["pt_keep"][low] and flt["pt_kept"][low] == 3 and 0 <= flt["pt_angle"][low] < np.deg2rad(1.5)
        assert not r["solvable"][behind] and r["solvable"][low] and flt["zero_weight"] == 1
        host, f, k = c["outlier"]
        row = int(c["scene"]["frame_off"][f]) + k
        o = int(np.nonzero(c["problem"].obs_row == row)[0][0])
        assert not flt["obs_keep"][o] and flt["pt_keep"][ids.index(host)] and flt["filtered_observations"] == 2
    if name == "frozen_all":
        assert not r["cg_iterations"].any() and np.array_equal(r["table"], c["problem"].table) and r["final_cost"] < r["initial_cost"]
    if name == "zero":
        assert np.array_equal(r["table"], c["problem"].table) and np.array_equal(r["xyz"], c["problem"].xyz) and r["termination"] == "max_iters"
    if name == "ring":
        assert sorted(np.diff(c["problem"].pt_off).tolist())[-3:] == [63, 64, 65] and {2, 3, 17} <= set(np.diff(c["problem"].pt_off).tolist())
    if name == "frames":
        assert np.diff(c["problem"].frm_off).tolist()[:6] == [0, 1, 63, 64, 65, 257]


# ---------------------------------------------------------------- the host side, ops replaced by the restatement
class StubOps:
    """pram_amd.ops as far as bundle.py and triangulation.frame_table use it, on CPU tensors, computed by the restatements."""

    def __init__(self):
        from pram_amd import ops
        for k in dir(ops):
            if k.startswith("BA_") or k in ("TRI_FRAME_COLS", "POSE_CAM_PARAMS", "_lib"):
                setattr(self, k, getattr(ops, k))
        self.calls = []

    def tri_frames(self, qvec, tvec, cam_model, cam_params, cam_model_host):
        F = len(cam_model_host)
        return torch.from_numpy(TR.frame_table(qvec.numpy()[:F], tvec.numpy()[:F], cam_model.numpy()[:F], cam_params.numpy()[:F]))

    def tri_normalize(self, keypoints, frame_off, cam_model, cam_params, cam_model_host, n_rows, off):
        F = len(cam_model_host)
        return torch.from_numpy(TR.normalize(keypoints.numpy()[:n_rows], frame_off.numpy()[:F + 1], cam_model.numpy()[:F], cam_params.numpy()[:F], off))

    def ba_begin(self, keypoints, cam_model, cam_params, cam_model_host, table, xyz, obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen,
                 n_points, n_obs, n_rows, max_iters, **kw):
        self.calls.append("ba_begin")
        F = len(cam_model_host)
        tabs = {"obs_row": obs_row.numpy()[:n_obs], "obs_frame": obs_frame.numpy()[:n_obs], "obs_point": obs_point.numpy()[:n_obs],
                "frm_off": frm_off.numpy()[:F + 1], "pt_off": pt_off.numpy()[:n_points + 1], "pt_obs": pt_obs.numpy()[:n_obs]}
        pr = BR.Problem(keypoints.numpy()[:n_rows], cam_model.numpy()[:F], cam_params.numpy()[:F], table.numpy()[:F], xyz.numpy()[:n_points], tabs,
                        frozen.numpy()[:F])
        views = {"state_i32": torch.zeros(self.BA_STATE_I32 + 2 * max_iters, dtype=torch.int32), "state_f64": torch.zeros(self.BA_STATE_F64, dtype=torch.float64),
                 "point_ok": torch.ones(n_points, dtype=torch.int32)}
        return {"problem": pr, "params": {"max_iters": max_iters, **kw}, "views": views, "n_frames": F, "n_points": n_points, "n_obs": n_obs,
                "max_iters": max_iters, "result": None}

    def ba_iterate(self, prob, n_iters, cg_iters, stages=31):
        self.calls.append("ba_iterate")
        if prob["result"] is not None:
            return
        r = prob["result"] = BR.run(prob["problem"], cg_iters=cg_iters, **prob["params"])
        si, sd, K, n = prob["views"]["state_i32"], prob["views"]["state_f64"], prob["max_iters"], len(r["accepted"])
        si[self.BA_SI_DONE], si[self.BA_SI_REASON] = 1, {"max_iters": 1, "ftol": 2}[r["termination"]]
        si[self.BA_SI_LM_ITER], si[self.BA_SI_ACCEPTED] = n, int(r["accepted"].sum())
        si[self.BA_STATE_I32:self.BA_STATE_I32 + n] = torch.from_numpy(r["cg_iterations"].astype(np.int32))
        si[self.BA_STATE_I32 + K:self.BA_STATE_I32 + K + n] = torch.from_numpy(r["accepted"].astype(np.int32))
        sd[self.BA_SD_COST], sd[self.BA_SD_COST0], sd[self.BA_SD_LAM] = r["final_cost"], r["initial_cost"], r["lam"]
        prob["views"]["point_ok"] = torch.from_numpy(r["solvable"].astype(np.int32))

    def ba_finish(self, prob, qvec, tvec, max_reproj_error=4.0, min_tri_angle=0.026179938779914945):
        self.calls.append("ba_finish")
        pr, p = prob["problem"], prob["params"]
        r = prob["result"] or BR.run(pr, **{**p, "max_iters": 0})
        if prob["result"] is None:
            sd = prob["views"]["state_f64"]
            sd[self.BA_SD_COST], sd[self.BA_SD_COST0], sd[self.BA_SD_LAM] = r["final_cost"], r["initial_cost"], r["lam"]
            prob["views"]["state_i32"][self.BA_SI_REASON] = 1
        flt = BR.filter_points(pr, r["table"], r["xyz"], max_reproj_error, float(np.rad2deg(min_tri_angle)), p.get("loss_scale", 1.0))
        q, t = qvec.numpy()[:pr.F].copy(), tvec.numpy()[:pr.F].copy()
        for f in np.nonzero(r["moved"])[0].tolist():
            q[f], t[f] = PR.rot_to_qvec(r["table"][f, :9].reshape(3, 3)), r["table"][f, 9:12]
        T = torch.from_numpy
        return {"qvec": T(q), "tvec": T(t), "xyz": T(r["xyz"].copy()), "obs_keep": T(flt["obs_keep"].astype(np.uint8)), "obs_error": T(flt["obs_error"]),
                "pt_keep": T(flt["pt_keep"].astype(np.int32)), "pt_error": T(flt["pt_error"]), "pt_angle": T(flt["pt_angle"]),
                "pt_kept": T(flt["pt_kept"].astype(np.int32)), "counts": torch.tensor([flt["zero_weight"], flt["filtered_observations"]], dtype=torch.int32)}


@pytest.fixture()
def stubbed(monkeypatch):
    from pram_amd.localization import bundle as BA
    from pram_amd.localization import triangulation as TG
    stub = StubOps()
    monkeypatch.setattr(TG, "ops", stub)
    monkeypatch.setattr(BA, "ops", stub)
    monkeypatch.setattr(TG, "_device", lambda device: torch.device("cpu"))
    return BA, stub


def _args(c):
    s = c["scene"]
    return s["frames"], s["cameras"], (s["qvec"], s["tvec"]), c["model"]


def test_host_logic_with_ops_stubbed(stubbed):
    BA, stub = stubbed
    c, r = BR.gpu_case("special"), BR.gpu_run("special")
    m = BA.bundle_adjust(*_args(c), "cpu", frozen=c["frozen"])
    assert stub.calls[0] == "ba_begin" and stub.calls[-1] == "ba_finish" and stub.calls.count("ba_iterate") == 1      # done after the first group
    rep, flt, ids = m["report"], r["filter"], c["model"]["point_ids"]
    assert rep["termination"] == r["termination"] and rep["lm_iterations"] == len(r["accepted"]) and rep["lm_accepted"] == int(r["accepted"].sum())
    assert rep["cg_iterations"].tolist() == r["cg_iterations"].tolist() and rep["accepted"].tolist() == r["accepted"].tolist()
    assert rep["initial_cost"] == r["initial_cost"] and rep["final_cost"] == r["final_cost"] and rep["lam"] == r["lam"]
    assert (rep["observations"], rep["zero_weight_observations"], rep["filtered_observations"], rep["filtered_points"], rep["unsolvable_points"]) == \
        (c["problem"].O, 1, 2, 2, 1)
    # ---- the model: ids preserved, filtered points and observations gone, everything else refined
    assert m["point_ids"].tolist() == ids[flt["pt_keep"]].tolist() and sorted(m["removed_ids"].tolist()) == sorted([c["behind"], c["low_angle"]])
    assert np.array_equal(m["point3D_xyzs"], r["xyz"][flt["pt_keep"]]) and np.array_equal(m["track_error"], flt["pt_error"][flt["pt_keep"]])
    host, f, k = c["outlier"]
    assert (f, k) not in set(zip(*[a.tolist() for a in m["tracks"][host]])) and len(m["tracks"][host][0]) == len(c["model"]["tracks"][host][0]) - 1
    assert set(m["tracks"]) == set(m["point_ids"].tolist()) == set(m["point3D_frame_ids"])
    assert sum(len(t[0]) for t in m["tracks"].values()) == int(flt["obs_keep"].sum()) - int((flt["obs_keep"] & ~flt["pt_keep"][c["problem"].obs_point]).sum())
    assert m["qvecs"].shape == (12, 4) and m["tvecs"].shape == (12, 3)
    assert np.array_equal(m["qvecs"][0], c["scene"]["qvec"][0]) and np.array_equal(m["tvecs"][11], c["scene"]["tvec"][11]) and not np.array_equal(m["qvecs"][3], c["scene"]["qvec"][3])
    assert np.allclose(TR.frame_table(m["qvecs"], m["tvecs"], c["scene"]["cam_model"], c["scene"]["cam_params"]), r["table"], atol=1e-12)
    # ---- a model with frames (map_tables') comes back with them cleaned, and goes on into the next stage's shapes
    from pram_amd.localization import outliers
    full = dict(c["model"])
    fo = c["scene"]["frame_off"]
    pid = np.full(int(fo[-1]), -1, dtype=np.int64)
    pid[c["problem"].obs_row] = ids[c["problem"].obs_point]
    full["frames"] = [{"point3D_ids": pid[a:b], "xyzs": np.zeros((b - a, 3))} for a, b in zip(fo[:-1], fo[1:])]
    m2 = BA.bundle_adjust(*_args(c)[:3], full, "cpu", frozen=c["frozen"])
    got = np.concatenate([fr["point3D_ids"] for fr in m2["frames"]])
    assert int((got >= 0).sum()) == sum(len(t[0]) for t in m2["tracks"].values()) and not np.isin(got, m2["removed_ids"]).any()
    for fr in m2["frames"]:
        has = fr["point3D_ids"] >= 0
        lookup = dict(zip(m2["point_ids"].tolist(), m2["point3D_xyzs"]))
        assert all(np.array_equal(x, lookup[i]) for i, x in zip(fr["point3D_ids"][has].tolist(), fr["xyzs"][has])) and not fr["xyzs"][~has].any()
    assert outliers.restrict_model(m2, np.ones(len(m2["point_ids"]), dtype=bool))["point_ids"].tolist() == m2["point_ids"].tolist()
    # ---- max_iters = 0: bit for bit; the gauge; the errors on their own
    z = BA.bundle_adjust(*_args(c), "cpu", max_iters=0)
    assert np.array_equal(z["qvecs"], c["scene"]["qvec"]) and np.array_equal(z["tvecs"], c["scene"]["tvec"]) and z["report"]["lm_iterations"] == 0
    assert np.array_equal(z["point3D_xyzs"], c["model"]["point3D_xyzs"][BR.gpu_run("zero")["filter"]["pt_keep"]]) and z["report"]["termination"] == "max_iters"
    fo_ = c["tables"]["frm_off"]
    assert BA.gauge_mask("colmap", None, fo_).tolist() == [63, 8] + [0] * 10 and not BA.gauge_mask("none", None, fo_).any()
    assert BA.gauge_mask("colmap", None, np.array([0, 0, 5, 5, 9])).tolist() == [0, 63, 0, 8] and BA.gauge_mask("colmap", c["frozen"], fo_).tolist() == c["frozen"].tolist()
    e = BA.reprojection_errors(*_args(c), "cpu")
    assert np.array_equal(e["error"], BR.gpu_run("zero")["filter"]["obs_error"]) and e["front"].sum() == c["problem"].O - 1
    assert np.array_equal(e["frame"], c["problem"].obs_frame) and np.array_equal(e["point_id"], ids[c["problem"].obs_point])
    # ---- refusals
    for bad in (dict(trials=3), dict(max_iter=3)):
        with pytest.raises(TypeError):
            BA.bundle_adjust(*_args(c), "cpu", **bad)
    for bad in (dict(cg_tol=0.0), dict(cg_tol=float("nan")), dict(loss_scale=-1.0), dict(max_iters=-1), dict(max_iters=2.5), dict(gauge="fixed"),
                dict(frozen=np.full(12, 64)), dict(frozen=np.zeros(11, dtype=int)), dict(frozen=np.zeros(12)), dict(lam0=float("inf"))):
        with pytest.raises(ValueError):
            BA.bundle_adjust(*_args(c), "cpu", **bad)
    broken = dict(c["model"], point3D_xyzs=np.where(np.arange(len(ids))[:, None] == 0, np.nan, c["model"]["point3D_xyzs"]))
    with pytest.raises(ValueError):
        BA.bundle_adjust(*_args(c)[:3], broken, "cpu")
    twice = dict(c["model"], tracks={**c["model"]["tracks"], int(ids[0]): c["model"]["tracks"][int(ids[1])]})
    with pytest.raises(ValueError):
        BA.bundle_adjust(*_args(c)[:3], twice, "cpu")
    with pytest.raises(ValueError):
        BA.bundle_adjust(c["scene"]["frames"], c["scene"]["cameras"], (c["scene"]["qvec"] * np.nan, c["scene"]["tvec"]), c["model"], "cpu")
    # ---- an empty model
    empty = {"point_ids": np.zeros(0, dtype=np.int64), "point3D_xyzs": np.zeros((0, 3)), "track_error": np.zeros(0), "tracks": {}, "point3D_frame_ids": {}}
    m0 = BA.bundle_adjust(*_args(c)[:3], empty, "cpu")
    assert m0["report"]["termination"] == "empty" and np.array_equal(m0["qvecs"], c["scene"]["qvec"]) and len(m0["point_ids"]) == 0


def test_no_cpu_path():
    from pram_amd._lib import PramHipError
    from pram_amd.localization import bundle as BA
    c = BR.gpu_case("two")
    with pytest.raises(PramHipError):
        BA.bundle_adjust(*_args(c), "cpu")
