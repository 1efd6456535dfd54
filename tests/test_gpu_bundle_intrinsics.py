"""GPU: the bundle adjustment with camera groups (bundle_adjust's refine flags, csrc/bundle.hip's pram_bac_* entries) against the
numpy restatement tests/bundle_intr_ref.py, stage by stage and end to end, on the runs of bundle_intr_ref.GPU_RUNS
(tests/test_bundle_intrinsics_cpu.py says what each is there for and asserts the margins that make the discrete results here
exact).  Every figure is printed before it is asserted; profiles/bundle_intrinsics_parity.md has the measured deviations behind
the bars."""
import numpy as np
import pytest
import torch

from tests import bundle_intr_ref as IR
from tests import bundle_ref as BR
from tests import triangulation_ref as TR

pytestmark = pytest.mark.gpu

SUM_BAR = 1e-12       # single-pass quantities, relative to the largest entry of the array compared (tests/test_gpu_bundle.py's bar)
# End results, device against restatement: ten times the largest deviation measured over the five runs
# (profiles/bundle_intrinsics_parity.md), all far under the ceilings of 1e-6 degrees, 1e-9 of the scene's extent, 1e-9 relative for
# focal lengths and principal points and 1e-9 absolute for distortion coefficients.  The single-pass quantities agree to the bit
# but for the Cholesky solves; what is left is the rounding of sin, cos and log1p and what the iterations make of it, which is why
# the runs are short (bundle_intr_ref.RUN_PARAMS says more).  Where the measurement is 0 the bar is ten ulps.
ROT_BAR = 1.1e-11         # degrees; measured 1.10e-12 (frames)
CENTRE_BAR = 6.7e-14      # relative to the scene's extent; measured 6.70e-15 (frames)
POINT_BAR = 7.7e-12       # relative to the scene's extent; measured 7.61e-13 (models: the point 420 away)
FOCAL_BAR = 1.6e-14       # focal lengths and principal points, relative; measured 1.55e-15 (models)
EXTRA_BAR = 4.0e-11       # distortion coefficients, absolute; measured 3.97e-12 (ring)
COST0_BAR = 2.3e-15       # the initial cost, relative; measured 0
COST_BAR = 7.6e-14        # the final cost, relative; measured 7.53e-15 (split)
OBS_ERR_BAR = 8.9e-12     # pixels; measured 8.87e-13 (models)
STAGED = sorted(IR.GPU_RUNS)


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def BA():
    from pram_amd.localization import bundle
    return bundle


def _args(c):
    s = c["scene"]
    return s["frames"], s["cameras"], (s["qvec"], s["tvec"]), c["model"]


def _params(c):
    return {**BR.DEFAULTS, **c["params"]}


def _group_tables(gp) -> dict:
    return {"frm_grp": gp.frm_grp.astype(np.int32), "grp_off": gp.grp_off.astype(np.int32), "grp_frame": gp.grp_frame.astype(np.int32),
            "grp_params": gp.k0.copy(), "grp_mask": gp.mask_in.astype(np.int32)}


def _begin(BA, c, dev, groups=None):
    """The device problem of a case, as bundle_adjust builds it (groups: other group tables, for the refusals)."""
    from pram_amd import ops
    from pram_amd.localization import triangulation as TG
    s, p = c["scene"], _params(c)
    table = TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), dev)
    tabs, gp = c["tables"], c["problem"]
    pr = gp.pr
    d = {k: TG._up(tabs[k], dev) for k in BA.TABLE_KEYS}
    g = {k: TG._up(v, dev) for k, v in (groups or _group_tables(gp)).items()}
    mask = BA.gauge_mask("colmap", c["frozen"], tabs["frm_off"])
    prob = ops.bac_begin(table["keypoints"], table["cam_model"], table["cam_model_host"], table["frames"], TG._up(pr.xyz, dev), d["obs_row"],
                         d["obs_frame"], d["obs_point"], d["frm_off"], d["pt_off"], d["pt_obs"], TG._up(mask, dev), g["frm_grp"], g["grp_off"],
                         g["grp_frame"], g["grp_params"], g["grp_mask"], pr.P, pr.O, table["n_rows"], gp.G, p["max_iters"],
                         loss_scale=p["loss_scale"], lam0=p["lam0"], cg_tol=p["cg_tol"], ftol=p["ftol"])
    return ops, prob, table


def _rel(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a - b).max() if a.size else 0.0)


@pytest.mark.parametrize("name", STAGED)
def test_single_pass_quantities(BA, dev, name):
    c = IR.gpu_case(name)
    gp, p = c["problem"], _params(c)
    pr = gp.pr
    ops, prob, _ = _begin(BA, c, dev)
    v = prob["views"]
    get = lambda k: v[k].cpu().numpy()
    lam = p["lam0"]
    J, ok, _ = IR.linearise(gp, pr.table, pr.xyz, gp.k0, p["loss_scale"])
    J20 = J[:, IR._J20]
    Vinv, g_p, good = BR.point_blocks(pr, J20, ok, lam)
    S, dU, b = BR.frame_blocks(pr, J20, Vinv, g_p, lam)
    Sg, dUg, bg, part = IR.group_blocks(gp, J, Vinv, g_p, lam)
    x, xg, n, tr = IR.pcg(gp, J, Vinv, S, Sg, dU, dUg, b, bg, lam, 1, p["cg_tol"])
    first = tr["first"]
    ops.bac_iterate(prob, 1, 0, ops.BA_STAGE_LINEARISE | ops.BA_STAGE_BLOCKS | ops.BA_STAGE_CG_INIT)
    sd = get("state_f64")
    fig = {"initial cost": abs(sd[ops.BA_SD_COST0] - IR.cost(gp, pr.table, pr.xyz, gp.k0, p["loss_scale"])) / max(sd[ops.BA_SD_COST0], 1e-300),
           "rows of 36": _rel(get("jac"), J), "V^-1": _rel(get("v_inv"), Vinv), "g_p": _rel(get("g_p"), g_p), "S blocks": _rel(get("s_block"), S),
           "diag U": _rel(get("diag_u"), dU), "b": _rel(get("b"), b), "frames' group sums": _rel(get("frame_group_sums"), part),
           "group blocks": _rel(get("g_block"), Sg), "diag U_k": _rel(get("g_diag_u"), dUg), "b_k": _rel(get("g_b"), bg),
           "z = M^-1 b": _rel(get("cg_z"), first["z"]), "z_k": _rel(get("g_cg_z"), first["zg"]),
           "r.z": abs(sd[3] - first["rz"]) / abs(first["rz"]), "b.b": abs(sd[7] - first["bb"]) / abs(first["bb"])}
    exact = np.array_equal(get("obs_ok").astype(bool), ok) and np.array_equal(get("point_ok").astype(bool), good) and \
        np.array_equal(get("frozen"), pr.fmask) and np.array_equal(get("grp_mask"), gp.gmask) and np.array_equal(get("grp_model"), gp.model) and \
        np.array_equal(get("grp_params"), gp.k0) and np.array_equal(get("cam_params"), gp.k0[gp.frm_grp])
    ops.bac_iterate(prob, 1, 1, ops.BA_STAGE_CG)
    sd = get("state_f64")
    fig.update({"q = S p": _rel(get("cg_q"), first["q"]), "q_k": _rel(get("g_cg_q"), first["qg"]), "p.q": abs(sd[4] - first["pap"]) / abs(first["pap"]),
                "x after one iteration": _rel(get("cg_x"), x), "x_k after one iteration": _rel(get("g_cg_x"), xg)})
    print(f"{name}: " + ", ".join(f"{k} {e:.2e}" for k, e in fig.items()) + f"; masks equal: {exact}")
    assert exact and all(e <= SUM_BAR for e in fig.values()), fig
    # a frozen or absent parameter: zero columns, a unit diagonal, a step of exactly 0
    jac, xs = get("jac"), get("g_cg_x")
    fz = gp.frozen_bits()
    og = gp.frm_grp[pr.obs_frame]
    for a in range(IR.NK):
        assert not jac[fz[og, a]][:, [12 + a, 20 + a]].any() and not xs[fz[:, a], a].any()


@pytest.fixture(scope="module")
def solved(BA, dev):
    """Every run once: (the case, the restatement, the device's outputs on the host, the report, the final table)."""
    cache = {}

    def get(name):
        if name not in cache:
            from pram_amd import ops
            c = IR.gpu_case(name)
            p = _params(c)
            ops_, prob, _ = _begin(BA, c, dev)
            state = prob["views"]["state_i32"]
            for _ in range(0, p["max_iters"], BA.BA_GROUP):
                ops.bac_iterate(prob, BA.BA_GROUP, p["cg_iters"])
                if int(state[ops.BA_SI_DONE].item()):
                    break
            s = c["scene"]
            out = ops.bac_finish(prob, torch.from_numpy(s["qvec"]).to(dev), torch.from_numpy(s["tvec"]).to(dev), max_reproj_error=p["max_reproj_error"],
                                 min_tri_angle=float(np.deg2rad(p["min_tri_angle"])))
            cache[name] = (c, IR.gpu_run(name), {k: t.cpu().numpy() for k, t in out.items()}, BA._report(prob, out, c["problem"].O),
                           prob["views"]["table"].cpu().numpy())
        return cache[name]
    return get


@pytest.mark.parametrize("name", STAGED)
def test_end_results(solved, name):
    c, r, out, rep, table = solved(name)
    gp, flt = c["problem"], r["filter"]
    pr = gp.pr
    extent = float(np.abs(c["truth"]["table"][:, 12:15]).max() * 2.0)
    rot, cen = BR.pose_errors(table, r["table"])
    k, kr = out["grp_params"], r["params"]
    lin = np.zeros_like(kr, dtype=bool)      # focal lengths and principal points: relative; the rest: absolute
    for q in range(gp.G):
        lin[q, list(IR.FOCAL[gp.model[q]] + IR.PP[gp.model[q]])] = True
    fig = {"rotation (degrees)": float(rot.max()), "centres / extent": float(cen.max() / extent),
           "points / extent": float(np.abs(out["xyz"] - r["xyz"]).max() / extent),
           "focal and principal point (relative)": float((np.abs(k - kr)[lin] / np.abs(kr[lin])).max()),
           "distortion (absolute)": float(np.abs(k - kr)[~lin].max()),
           "initial cost": abs(rep["initial_cost"] - r["initial_cost"]) / r["initial_cost"], "final cost": abs(rep["final_cost"] - r["final_cost"]) / r["final_cost"],
           "observation errors (px)": float(np.abs(out["obs_error"] - flt["obs_error"]).max())}
    print(f"{name}: accepted {rep['accepted'].astype(int).tolist()}, CG {rep['cg_iterations'].tolist()}, {rep['termination']}, lam {rep['lam']:.1e}; "
          + ", ".join(f"{k_} {e:.2e}" for k_, e in fig.items()))
    # ---- the discrete results: equal
    assert rep["accepted"].tolist() == r["accepted"].tolist() and rep["cg_iterations"].tolist() == r["cg_iterations"].tolist()
    assert rep["termination"] == r["termination"] and rep["lam"] == r["lam"] and rep["cg_breakdowns"] == 0
    assert np.array_equal(out["obs_keep"].astype(bool), flt["obs_keep"]) and np.array_equal(out["pt_keep"].astype(bool), flt["pt_keep"])
    assert np.array_equal(out["pt_kept"], flt["pt_kept"])
    # ---- the continuous ones: within the bars
    assert fig["rotation (degrees)"] <= ROT_BAR and fig["centres / extent"] <= CENTRE_BAR and fig["points / extent"] <= POINT_BAR
    assert fig["focal and principal point (relative)"] <= FOCAL_BAR and fig["distortion (absolute)"] <= EXTRA_BAR
    assert fig["initial cost"] <= COST0_BAR and fig["final cost"] <= COST_BAR and fig["observation errors (px)"] <= OBS_ERR_BAR
    # ---- what does not move does not move, bit for bit: frames, frozen and absent parameters, a group without observations
    still = ~r["moved"]
    assert np.array_equal(out["qvec"][still], c["scene"]["qvec"][still]) and np.array_equal(out["tvec"][still], c["scene"]["tvec"][still])
    assert np.array_equal(k[gp.frozen_bits()], gp.k0[gp.frozen_bits()])
    assert (k != gp.k0).any()


def _flag_kw(c) -> dict:
    return dict(zip(("refine_focal_length", "refine_principal_point", "refine_extra_params"), c["flags"]))


def test_flags_off_is_the_existing_path_bit_for_bit(BA, dev):
    c = BR.gpu_case("special")
    args = (c["scene"]["frames"], c["scene"]["cameras"], (c["scene"]["qvec"], c["scene"]["tvec"]), c["model"])
    a = BA.bundle_adjust(*args, dev, frozen=c["frozen"])
    grp = np.arange(len(args[0])) % 5
    for kw in ({"camera_groups": None}, {"camera_groups": grp}, {"camera_groups": grp, "refine_focal_length": False}):
        b = BA.bundle_adjust(*args, dev, frozen=c["frozen"], **kw)
        for key in ("qvecs", "tvecs", "point3D_xyzs", "track_error", "point_ids", "removed_ids"):
            assert np.array_equal(a[key], b[key]), key
        assert a["report"]["final_cost"] == b["report"]["final_cost"] and a["report"]["cg_iterations"].tolist() == b["report"]["cg_iterations"].tolist()
        assert b["report"]["intrinsics"] == [] and all(x is y for x, y in zip(b["cameras"], args[1]))
        assert np.array_equal(b["camera_groups"], grp)


def test_the_same_call_twice_is_bit_equal(BA, dev):
    c = IR.gpu_case("models")
    a = BA.bundle_adjust(*_args(c), dev, frozen=c["frozen"], **c["params"], **_flag_kw(c))
    b = BA.bundle_adjust(*_args(c), dev, frozen=c["frozen"], **c["params"], **_flag_kw(c))
    for k in ("qvecs", "tvecs", "point3D_xyzs", "track_error", "point_ids"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x[3], y[3]) for x, y in zip(a["cameras"], b["cameras"]))
    assert a["report"]["final_cost"] == b["report"]["final_cost"] and a["report"]["cg_iterations"].tolist() == b["report"]["cg_iterations"].tolist()
    # the public call runs the restated problem: the default grouping is the case's, the refined parameters the restatement's
    r, gp = IR.gpu_run("models"), c["problem"]
    assert np.array_equal(a["camera_groups"], c["frm_grp"]) and a["report"]["accepted"].tolist() == r["accepted"].tolist()
    for q, row in enumerate(a["report"]["intrinsics"]):
        n = IR.N_PARAMS[gp.model[q]]
        assert row["mask"] == gp.gmask[q] and row["observations"] == gp.n_obs[q] and np.array_equal(row["params_before"], gp.k0[q, :n])
        assert np.abs(row["params_after"] - r["params"][q, :n]).max() <= 1e-9 * np.abs(r["params"][q, :n]).max()
    assert all(len(cam[3]) == IR.N_PARAMS[gp.model[gp.frm_grp[f]]] for f, cam in enumerate(a["cameras"]))


def test_refusals(BA, dev):
    from pram_amd import ops
    from pram_amd._lib import PramHipError
    c = IR.gpu_case("split")
    gp = c["problem"]
    good = _group_tables(gp)

    def reason(groups):
        _, prob, _ = _begin(BA, c, dev, groups)
        ops.bac_iterate(prob, 2, 4)
        si = prob["views"]["state_i32"].cpu().numpy()
        return si[ops.BA_SI_DONE], ops.BA_REASONS[int(si[ops.BA_SI_REASON])], si[ops.BA_SI_LM_ITER]

    assert reason(good)[1] != "tables"
    # deliberately inconsistent group tables end the run on the device before anything reads through them
    f_out = {**good, "grp_frame": good["grp_frame"].copy()}
    f_out["grp_frame"][2] = gp.F + 1000                 # a frame out of range
    twice = {**good, "grp_frame": good["grp_frame"].copy()}
    twice["grp_frame"][1] = twice["grp_frame"][0]       # a frame in its group twice, another in none
    wrong = {**good, "frm_grp": good["frm_grp"].copy()}
    wrong["frm_grp"][0] = 10 ** 6                        # a group out of range
    mixed = {**good, "frm_grp": good["frm_grp"].copy(), "grp_frame": np.array([0, 2, 4, 6, 9, 1, 3, 5, 7, 8], dtype=np.int32),
             "grp_off": np.array([0, 5, 9, 10, 10], dtype=np.int32)}
    mixed["frm_grp"][9], mixed["frm_grp"][8] = 0, 2      # frame 9 (SIMPLE_RADIAL) in a RADIAL group: two models in one group
    offs = {**good, "grp_off": np.array([0, 4, 3, 9, 10], dtype=np.int32)}
    for name, g in (("frame out of range", f_out), ("frame twice", twice), ("group out of range", wrong), ("two models", mixed), ("offsets", offs)):
        done, why, its = reason(g)
        print(f"{name}: done {done}, reason {why}, iterations {its}")
        assert done == 1 and why == "tables" and its == 0, name
    L = ops._lib.load()
    assert L.pram_bac_workspace_bytes(4, 1, 1, 5, 1) == 0 and L.pram_bac_workspace_bytes(4, 1, 1, 0, 1) == 0 and L.pram_bac_workspace_bytes(4, 1, 1, 2, 5000) == 0
    with pytest.raises(PramHipError):
        ops.bac_iterate({"context": __import__("ctypes").create_string_buffer(ops.BAC_CONTEXT_BYTES)}, 1, 1)
    # the host's refusals
    args = _args(c)
    for bad in (np.zeros(3, dtype=np.int64), np.zeros(gp.F), -np.ones(gp.F, dtype=np.int64), np.zeros(gp.F, dtype=np.int64)):
        with pytest.raises(ValueError):
            BA.bundle_adjust(*args, dev, camera_groups=bad, refine_focal_length=True)
    with pytest.raises(ValueError):
        BA.bundle_adjust(*args, dev, refine_focal_length=1)


def test_end_to_end_recovery(BA, dev):
    """The planted recovery scene (0.5 px noise, 3 % gross outliers) through bundle_adjust with refine_focal_length and
    refine_extra_params, then triangulate_map again with the returned cameras and poses: against the constant-intrinsics run of the
    same data, no fewer points and a smaller mean track error, in the adjusted model and in the one triangulated again."""
    c = IR.recovery_case(noise=0.5, outliers=0.03)
    args = _args(c)
    off = BA.bundle_adjust(*args, dev, frozen=c["frozen"])
    on = BA.bundle_adjust(*args, dev, frozen=c["frozen"], refine_focal_length=True, refine_extra_params=True)
    truth = c["truth"]
    f_true = np.array([cam[3][0] for cam in truth["cameras"]])
    f_in, f_out = np.array([cam[3][0] for cam in args[1]]), np.array([cam[3][0] for cam in on["cameras"]])
    k_out, k_true = np.array([cam[3][3] for cam in on["cameras"]]), np.array([cam[3][3] for cam in truth["cameras"]])
    e_on = BA.reprojection_errors(args[0], on["cameras"], (on["qvecs"], on["tvecs"]), on, dev)["error"]
    e_off = BA.reprojection_errors(args[0], off["cameras"], (off["qvecs"], off["tvecs"]), off, dev)["error"]
    print(f"flags off: cost {off['report']['final_cost']:.1f}, {len(off['point_ids'])} points, mean track error {off['track_error'].mean():.3f} px, "
          f"mean observation error {e_off.mean():.3f} px; flags on: cost {on['report']['final_cost']:.1f}, {len(on['point_ids'])} points, mean track "
          f"error {on['track_error'].mean():.3f} px, mean observation error {e_on.mean():.3f} px, CG {on['report']['cg_iterations'].tolist()}; focal "
          f"error {np.abs(f_in / f_true - 1).max():.3%} -> {np.abs(f_out / f_true - 1).max():.3%}, k1 error {np.abs(k_out - k_true).max():.2e}")
    assert len(on["point_ids"]) >= len(off["point_ids"]) and on["track_error"].mean() < off["track_error"].mean()
    assert on["report"]["final_cost"] < off["report"]["final_cost"]
    assert np.abs(f_out / f_true - 1).max() < np.abs(f_in / f_true - 1).max()
    # the same map triangulated again from the refined poses, once with the returned cameras and once with the input's
    from pram_amd.localization import triangulation as TG
    pairs = [(a, b) for a in range(len(args[0])) for b in range(a + 1, min(a + 3, len(args[0])))]
    where = truth["where"]
    pts = sorted({p for _, p in where})
    matches = [np.array([(where[(a, p)], where[(b, p)]) for p in pts if (a, p) in where and (b, p) in where], dtype=np.int64).reshape(-1, 2) for a, b in pairs]
    t_on = TG.triangulate_map(args[0], on["cameras"], (on["qvecs"], on["tvecs"]), pairs, matches, dev)
    t_off = TG.triangulate_map(args[0], off["cameras"], (off["qvecs"], off["tvecs"]), pairs, matches, dev)
    print(f"triangulated again: flags off {len(t_off['point_ids'])} points, mean track error {t_off['track_error'].mean():.3f} px; "
          f"flags on {len(t_on['point_ids'])} points, mean track error {t_on['track_error'].mean():.3f} px")
    assert len(t_on["point_ids"]) >= len(t_off["point_ids"]) and t_on["track_error"].mean() < t_off["track_error"].mean()


def test_reconstruct_refines_rough_focal_lengths(dev):
    """mapper.reconstruct on mapper_ref's planted scene with the focal lengths started 3 % off: bundle=dict(refine_focal_length=True)
    reaches the final adjustment, the result carries cameras, and their focal lengths are closer to the planted ones."""
    from pram_amd.localization import mapper
    from tests import mapper_ref as MR
    s = MR.planted_scene()
    rough = [IR._scaled(cam, 1.03) for cam in s["cameras"]]
    res = mapper.reconstruct(s["frames"], rough, s["pairs"], s["matches"], dev, bundle=dict(refine_focal_length=True))
    assert res["report"]["success"] and len(res["cameras"]) == len(rough)
    m = [int(IR.PR.camera_row(cam)[0]) for cam in s["cameras"]]
    foc = lambda cams: np.array([np.mean([cam[3][a] for a in IR.FOCAL[mi]]) for cam, mi in zip(cams, m)])
    reg = res["registered"]
    before, after = np.abs(foc(rough) / foc(s["cameras"]) - 1)[reg], np.abs(foc(res["cameras"]) / foc(s["cameras"]) - 1)[reg]
    print(f"reconstruct: {int(reg.sum())} frames registered, focal error mean {before.mean():.3%} -> {after.mean():.3%}, max {before.max():.3%} -> "
          f"{after.max():.3%}; final BA CG {res['report']['final_ba']['cg_iterations'].tolist()}")
    assert after.mean() < before.mean()
