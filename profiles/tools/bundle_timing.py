"""Time of every stage of the bundle adjustment (pram_amd/localization/bundle.py, csrc/bundle.hip) on a simulated map of
production size, of one conjugate-gradient iteration against the bytes it must move, and of the whole call; writes
profiles/bundle_timing.md.

    python profiles/tools/bundle_timing.py [--frames 2000] [--points 100000] [--reps 10] [--out FILE]
    python profiles/tools/bundle_timing.py --intrinsics [...]      # writes profiles/bundle_intrinsics_timing.md instead

--intrinsics times the adjustment with camera groups (refine_focal_length: one group, the street's one camera) beside the one
with constant intrinsics on the same map, in the same process, interleaved repetition by repetition: one LM iteration without its
CG iterations, one CG iteration, and the whole call of each.

The map: --frames pinhole cameras (640 x 480, f = 500) half a metre apart along a street, looking sideways; --points points 4 to
12 m away, each seen by about eight of the frames around it with 0.5 px noise; the poses drift (a random walk of 0.02 degrees and
2 mm per frame) and the points start 5 cm off.  Every stage is warmed up; then --reps repetitions between HIP events on the
current stream, medians with the smallest and largest value; the whole bundle_adjust call (tables, uploads, the iterations, the
filter, one read-back) by a host clock around work that ends in a device synchronise.  The compiler's resource report per kernel
comes from compiling csrc/bundle.hip once more with -Rpass-analysis=kernel-resource-usage (no device needed).  A second table
runs the whole call under other budgets (max_iters, cg_iters).  There is no parent to compare with: the file states times, no
bar.  The section "Reading" of the committed file was written by hand after the run and is not produced here."""
from __future__ import annotations

import argparse
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def resources() -> list:
    """(kernel, VGPRs, scratch bytes per lane, static LDS bytes, occupancy in waves per SIMD) per kernel of bundle.hip"""
    from pram_amd import build
    src = build.CSRC / "bundle.hip"
    r = subprocess.run([build.HIPCC, *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", "/dev/null"],
                       capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"(bac?_\w+?_kernel|ransac_pick_kernel)", m.group(1))
            cur = {"name": (name.group(1) + ("<Bac>" if "INS_3BacE" in m.group(1) else "")) if name else m.group(1)}
            rows.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("spill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return [r for r in rows if r["name"].startswith(("ba_", "bac_"))]


def simulate(n_frames: int, n_points: int, seed: int = 0) -> dict:
    """-> frames, cameras, the drifted poses, the true ones and the model (triangulate_map's shape), all by numpy."""
    rng = np.random.RandomState(seed)
    step, f0, w, h = 0.5, 500.0, 640, 480
    cx = np.arange(n_frames) * step
    X = np.stack([rng.uniform(0.0, cx[-1], n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(4.0, 12.0, n_points)], 1)
    near = np.rint(X[:, 0] / step).astype(np.int64)
    offs = np.arange(-8, 9)
    fr = near[:, None] + offs[None]
    u = f0 * (X[:, None, 0] - fr * step) / X[:, None, 2] + w / 2
    v = np.broadcast_to(f0 * X[:, None, 1] / X[:, None, 2] + h / 2, u.shape)
    vis = (fr >= 0) & (fr < n_frames) & (u >= 8) & (u < w - 8) & (v >= 8) & (v < h - 8) & (rng.uniform(size=u.shape) < 0.6)
    pt, k = np.nonzero(vis)
    frame = fr[pt, k]
    px = np.stack([u[pt, k], v[pt, k]], 1) - 0.5 + rng.normal(size=(pt.shape[0], 2)) * 0.5
    order = np.lexsort((pt, frame))
    pt, frame, px = pt[order], frame[order], px[order].astype(np.float32)
    off = np.searchsorted(frame, np.arange(n_frames + 1))
    kpt = np.arange(pt.shape[0]) - off[frame]
    frames = [{"keypoints": px[a:b]} for a, b in zip(off[:-1], off[1:])]
    cameras = [("SIMPLE_PINHOLE", w, h, [f0, w / 2.0, h / 2.0])] * n_frames
    by_pt = np.argsort(pt, kind="stable")
    cnt = np.bincount(pt, minlength=n_points)
    keep = np.nonzero(cnt >= 2)[0]
    starts = np.concatenate([[0], np.cumsum(cnt)])
    tracks = {int(p) + 1: (frame[by_pt[starts[p]:starts[p + 1]]], kpt[by_pt[starts[p]:starts[p + 1]]]) for p in keep.tolist()}
    q_true, t_true = np.tile([1.0, 0.0, 0.0, 0.0], (n_frames, 1)), np.stack([-cx, np.zeros(n_frames), np.zeros(n_frames)], 1)
    w_drift = np.cumsum(rng.normal(size=(n_frames, 3)) * np.deg2rad(0.02), 0)
    c_drift = np.cumsum(rng.normal(size=(n_frames, 3)) * 0.002, 0)
    w_drift[0] = c_drift[0] = 0.0
    th = np.linalg.norm(w_drift, axis=1)
    axis = w_drift / np.where(th > 0, th, 1.0)[:, None]
    q = np.concatenate([np.cos(th / 2)[:, None], axis * np.sin(th / 2)[:, None]], 1)
    from tests import pose_ref as PR
    t = np.stack([-PR.qvec_to_rot(q[f]) @ (np.array([cx[f], 0.0, 0.0]) + c_drift[f]) for f in range(n_frames)])
    model = {"point_ids": keep + 1, "point3D_xyzs": X[keep] + rng.normal(size=(keep.shape[0], 3)) * 0.05, "track_error": np.zeros(keep.shape[0]),
             "tracks": tracks, "point3D_frame_ids": {p: tk[0] for p, tk in tracks.items()}}
    return {"frames": frames, "cameras": cameras, "poses": (q, t), "true": (q_true, t_true), "model": model, "n_obs": int(sum(len(tk[0]) for tk in tracks.values()))}


def med(xs) -> str:
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def measure(sim: dict, reps: int) -> dict:
    import torch
    from pram_amd import ops
    from pram_amd.localization import bundle as BA
    from pram_amd.localization import triangulation as TG
    dev = torch.device("cuda:0")
    p = BA._ba_params("bundle_timing", {})
    qv, tv, ids, xyz, frame_ids = BA._inputs(sim["frames"], sim["poses"], sim["model"])
    t0 = time.perf_counter()
    table = TG.frame_table(sim["frames"], sim["cameras"], (qv, tv), dev)
    tabs = BA.observation_tables(sim["model"], frame_ids, table["frame_off_host"])
    torch.cuda.synchronize()
    t_tables = (time.perf_counter() - t0) * 1e3
    mask = BA.gauge_mask("colmap", None, tabs["frm_off"])
    d = {k: TG._up(tabs[k], dev) for k in BA.TABLE_KEYS}
    O, Pn, F = tabs["obs_row"].shape[0], xyz.shape[0], len(sim["frames"])

    def begin():
        return ops.ba_begin(table["keypoints"], table["cam_model"], table["cam_params"], table["cam_model_host"], table["frames"], TG._up(xyz, dev),
                            d["obs_row"], d["obs_frame"], d["obs_point"], d["frm_off"], d["pt_off"], d["pt_obs"], TG._up(mask, dev), Pn, O, table["n_rows"],
                            p["max_iters"], loss_scale=p["loss_scale"], lam0=p["lam0"], cg_tol=p["cg_tol"], ftol=p["ftol"])

    stages = (("begin (check, copies, initial cost)", None), ("linearise", ops.BA_STAGE_LINEARISE), ("blocks (points, frames)", ops.BA_STAGE_BLOCKS),
              ("CG start (preconditioner, dots)", ops.BA_STAGE_CG_INIT), ("one CG iteration", ops.BA_STAGE_CG),
              ("step (back-substitution, candidate, cost, decision, apply)", ops.BA_STAGE_STEP))
    times = {k: [] for k, _ in stages}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
    for rep in range(reps + 2):      # two warm-ups
        ev[0].record()
        prob = begin()
        ev[1].record()
        for i, (_, bits) in enumerate(stages[1:], start=1):
            ops.ba_iterate(prob, 1, 1, bits)
            ev[i + 1].record()
        torch.cuda.synchronize()
        if rep >= 2:
            for i, (k, _) in enumerate(stages):
                times[k].append(ev[i].elapsed_time(ev[i + 1]))
    whole, rep_last = [], None
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = BA.bundle_adjust(sim["frames"], sim["cameras"], sim["poses"], sim["model"], dev)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
        rep_last = res
    sweep = []
    for max_iters, cg_iters in ((40, 20), (40, 60), (40, 200), (100, 60), (100, 200)):      # what the budgets buy on this map
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = BA.bundle_adjust(sim["frames"], sim["cameras"], sim["poses"], sim["model"], dev, max_iters=max_iters, cg_iters=cg_iters)["report"]
        torch.cuda.synchronize()
        sweep.append((max_iters, cg_iters, (time.perf_counter() - t0) * 1e3, r))
    # the bytes one CG iteration must move: both passes read every observation's Jacobians and indices once
    jac = 2 * O * 18 * 8
    idx = O * (4 + 4) + O * 4
    vec = Pn * (6 + 3 + 3) * 8 + F * 6 * 8 * 9
    return {"times": times, "whole": whole, "tables_ms": t_tables, "sweep": sweep, "report": rep_last["report"], "res": rep_last, "bytes": jac + idx + vec, "O": O, "P": Pn,
            "F": F, "workspace": prob["workspace"].numel()}


def measure_intrinsics(sim: dict, reps: int) -> dict:
    """Flags off and on, interleaved: per repetition the stages of one LM iteration without CG and one CG iteration of each."""
    import torch
    from pram_amd import ops
    from pram_amd.localization import bundle as BA
    from pram_amd.localization import triangulation as TG
    dev = torch.device("cuda:0")
    p = BA._ba_params("bundle_timing", {"refine_focal_length": True})
    qv, tv, ids, xyz, frame_ids = BA._inputs(sim["frames"], sim["poses"], sim["model"])
    table = TG.frame_table(sim["frames"], sim["cameras"], (qv, tv), dev)
    tabs = BA.observation_tables(sim["model"], frame_ids, table["frame_off_host"])
    mask = TG._up(BA.gauge_mask("colmap", None, tabs["frm_off"]), dev)
    d = {k: TG._up(tabs[k], dev) for k in BA.TABLE_KEYS}
    gt = BA.group_tables(sim["cameras"], BA.camera_groups(sim["cameras"]), p)
    g = {k: TG._up(gt[k], dev) for k in BA.GROUP_KEYS}
    O, Pn, F, G = tabs["obs_row"].shape[0], xyz.shape[0], len(sim["frames"]), gt["grp_params"].shape[0]
    kw = dict(loss_scale=p["loss_scale"], lam0=p["lam0"], cg_tol=p["cg_tol"], ftol=p["ftol"])
    x = TG._up(xyz, dev)

    def begin(cam: bool):
        if cam:
            return ops.bac_begin(table["keypoints"], table["cam_model"], table["cam_model_host"], table["frames"], x, d["obs_row"], d["obs_frame"],
                                 d["obs_point"], d["frm_off"], d["pt_off"], d["pt_obs"], mask, g["frm_grp"], g["grp_off"], g["grp_frame"], g["grp_params"],
                                 g["grp_mask"], Pn, O, table["n_rows"], G, p["max_iters"], **kw)
        return ops.ba_begin(table["keypoints"], table["cam_model"], table["cam_params"], table["cam_model_host"], table["frames"], x, d["obs_row"],
                            d["obs_frame"], d["obs_point"], d["frm_off"], d["pt_off"], d["pt_obs"], mask, Pn, O, table["n_rows"], p["max_iters"], **kw)

    lm_bits = ops.BA_STAGE_LINEARISE | ops.BA_STAGE_BLOCKS | ops.BA_STAGE_CG_INIT
    times = {(cam, k): [] for cam in (False, True) for k in ("lm", "cg", "step")}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for rep in range(reps + 2):      # two warm-ups
        for cam in (False, True):
            it = ops.bac_iterate if cam else ops.ba_iterate
            prob = begin(cam)
            ev[0].record()
            it(prob, 1, 0, lm_bits)
            ev[1].record()
            it(prob, 1, 1, ops.BA_STAGE_CG)
            ev[2].record()
            it(prob, 1, 0, ops.BA_STAGE_STEP)
            ev[3].record()
            torch.cuda.synchronize()
            if rep >= 2:
                for i, k in enumerate(("lm", "cg", "step")):
                    times[(cam, k)].append(ev[i].elapsed_time(ev[i + 1]))
    whole = {False: [], True: []}
    reports = {}
    for rep in range(3):
        for cam in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = BA.bundle_adjust(sim["frames"], sim["cameras"], sim["poses"], sim["model"], dev, refine_focal_length=cam)
            torch.cuda.synchronize()
            whole[cam].append((time.perf_counter() - t0) * 1e3)
            reports[cam] = res["report"]
    return {"times": times, "whole": whole, "reports": reports, "O": O, "P": Pn, "F": F, "G": G}


def write_intrinsics(a, sim: dict, commit: str):
    m = measure_intrinsics(sim, a.reps)
    t, O = m["times"], m["O"]
    lines = ["# Bundle adjustment with camera groups: time per iteration, flags off and on", "",
             f"Measured {time.strftime('%Y-%m-%d')} on an MI355X by profiles/tools/bundle_timing.py --intrinsics, on top of commit {commit}.  Milliseconds, median "
             f"(smallest .. largest) of {a.reps} repetitions after two warm-ups, between HIP events; flags off (pram_ba_*) and on (pram_bac_*, "
             "refine_focal_length, one group: the street's one camera) in the same process, interleaved repetition by repetition.  No bar is set.", "",
             f"## {m['F']} frames, {m['G']} group, {m['P']} points, {m['O']} observations (the simulated street of profiles/bundle_timing.md)", "",
             "| | flags off | flags on | on / off |", "|---|---|---|---|"]
    for k, name in (("lm", "one LM iteration without CG: linearise, blocks, CG start"), ("step", "its step: back-substitution, candidate, cost, decision, apply"),
                    ("cg", "one CG iteration")):
        off, on = t[(False, k)], t[(True, k)]
        lines.append(f"| {name} | {med(off)} | {med(on)} | {statistics.median(on) / statistics.median(off):.2f} |")
    lines.append(f"| bundle_adjust, whole call | {med(m['whole'][False])} | {med(m['whole'][True])} | {statistics.median(m['whole'][True]) / statistics.median(m['whole'][False]):.2f} |")
    lines += ["", f"Derived, not measured: a CG iteration reads every observation's row twice; the row grows from 20 to 36 doubles (the 18 and 34 of them that are "
              f"Jacobians: {2 * O * 18 * 8 / 1e6:.0f} MB -> {2 * O * 34 * 8 / 1e6:.0f} MB a CG iteration here), and the matvec has one launch more (the groups' "
              "fold), the update and the direction one each.  The expected cost is that 36 / 20 growth of the traffic plus the launches.", ""]
    for cam in (False, True):
        r = m["reports"][cam]
        lines.append(f"Flags {'on' if cam else 'off'}: {r['lm_iterations']} LM iterations ({r['lm_accepted']} accepted, {r['termination']}), CG iterations per LM iteration "
                     f"{r['cg_iterations'].tolist()}; cost {r['initial_cost']:.1f} -> {r['final_cost']:.1f}; {r['cg_breakdowns']} CG breakdowns."
                     + (f"  Focal length {r['intrinsics'][0]['params_before'][0]:.3f} -> {r['intrinsics'][0]['params_after'][0]:.3f} (planted 500)." if cam else ""))
        lines.append("")
    lines += ["## What the compiler reports (gfx950, -O3)", "", "| kernel | VGPRs | VGPR spills | scratch bytes / lane | static LDS bytes | occupancy (waves / SIMD) |",
              "|---|---|---|---|---|---|"]
    for r in resources():
        lines.append(f"| {r['name']} | {r.get('vgpr')} | {r.get('spill')} | {r.get('scratch')} | {r.get('lds')} | {r.get('occ')} |")
    lines.append("")
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


def pose_error(res: dict, sim: dict) -> tuple:
    from tests import bundle_ref as BR
    from tests import triangulation_ref as TR
    n = len(sim["frames"])
    model, prm = np.zeros(n, dtype=np.int32), np.tile([500.0, 320.0, 240.0, 0, 0, 0, 0, 0], (n, 1))
    want = TR.frame_table(*sim["true"], model, prm)
    before, after = TR.frame_table(*sim["poses"], model, prm), TR.frame_table(res["qvecs"], res["tvecs"], model, prm)
    return BR.pose_errors(before, want), BR.pose_errors(after, want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--intrinsics", action="store_true")
    a = ap.parse_args()
    a.out = a.out or str(ROOT / "profiles" / ("bundle_intrinsics_timing.md" if a.intrinsics else "bundle_timing.md"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bundle_timing: no GPU (a time is measured on the device or not at all)")
    commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "working tree"
    sim = simulate(a.frames, a.points)
    if a.intrinsics:
        return write_intrinsics(a, sim, commit)
    m = measure(sim, a.reps)
    rep = m["report"]
    (r0, c0), (r1, c1) = pose_error(m["res"], sim)
    cg = statistics.median(m["times"]["one CG iteration"])
    lines = ["# Bundle adjustment: time per stage", "",
             f"Measured {time.strftime('%Y-%m-%d')} on an MI355X by profiles/tools/bundle_timing.py, on top of commit {commit}.  Milliseconds, median "
             f"(smallest .. largest) of {a.reps} repetitions after two warm-ups, the stages between HIP events; the whole call by a host clock around a "
             "device synchronise, three times.  There is no parent to compare with and no bar.", "",
             f"## {m['F']} frames, {m['P']} points, {m['O']} observations (simulated street)", "", "| stage | ms |", "|---|---|"]
    for k, v in m["times"].items():
        lines.append(f"| {k} | {med(v)} |")
    lines += [f"| bundle_adjust, whole call | {med(m['whole'])} |", f"| of it on the host before the first launch: frame table and observation tables | {m['tables_ms']:.1f} |", "",
              f"One CG iteration must move {m['bytes'] / 1e6:.1f} MB (the Jacobians of every observation twice, 144 B each, the indices, the per-point and "
              f"per-frame vectors): {m['bytes'] / 1e9 / (cg / 1e3):.1f} GB/s at the median, six launches.  Workspace {m['workspace'] / 2 ** 20:.1f} MiB.", "",
              f"The whole call ran {rep['lm_iterations']} LM iterations ({rep['lm_accepted']} accepted, {rep['termination']}), CG iterations per LM iteration "
              f"{rep['cg_iterations'].tolist()}; cost {rep['initial_cost']:.1f} -> {rep['final_cost']:.1f}; {rep['filtered_points']} points and "
              f"{rep['filtered_observations']} observations filtered, {rep['unsolvable_points']} points unsolvable, {rep['cg_breakdowns']} CG breakdowns.  Against "
              f"the planted poses (gauge: frame 0 and t_x of frame 1): rotation worst {r0.max():.3f} -> {r1.max():.3f} degrees, median {np.median(r0):.3f} -> "
              f"{np.median(r1):.3f}; centres worst {c0.max():.3f} -> {c1.max():.3f} m, median {np.median(c0):.3f} -> {np.median(c1):.3f}.", "",
              "## What the budgets buy on this map", "", "| max_iters | cg_iters | whole call, ms | LM iterations (accepted) | CG iterations, sum (largest) | final cost | termination |",
              "|---|---|---|---|---|---|---|"]
    for mi, ci, ms, r in m["sweep"]:
        cgs = r["cg_iterations"]
        lines.append(f"| {mi} | {ci} | {ms:.0f} | {r['lm_iterations']} ({r['lm_accepted']}) | {int(cgs.sum())} ({int(cgs.max()) if len(cgs) else 0}) | {r['final_cost']:.1f} | {r['termination']} |")
    lines += ["",
              "## What the compiler reports (gfx950, -O3)", "", "| kernel | VGPRs | VGPR spills | scratch bytes / lane | static LDS bytes | occupancy (waves / SIMD) |",
              "|---|---|---|---|---|---|"]
    for r in resources():
        lines.append(f"| {r['name']} | {r.get('vgpr')} | {r.get('spill')} | {r.get('scratch')} | {r.get('lds')} | {r.get('occ')} |")
    lines.append("")
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
