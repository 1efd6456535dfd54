"""Time of every stage of the two-view estimator (pram_amd/localization/twoview.py, csrc/twoview.hip) on planted pairs of a
production shape, and of one pair alone; writes profiles/twoview_timing.md.

    python profiles/tools/twoview_timing.py [--pairs 256] [--trials 1024] [--matches 500] [--reps 10] [--out FILE]

The batch: --pairs planted pairs (tests/twoview_ref.make_scene: two cameras of the five models in turn, --matches matches each,
30 % of them outliers, 0.5 px noise), one chunk.  Every shape is warmed up twice; then --reps repetitions, each stage between two
HIP events on the current stream (hypotheses; score with the pick; finish), and the whole estimate_two_view call, uploads and
read-back included, by a host clock around work that ends in a device synchronise; medians with the smallest and largest value.
The compiler's resource report per kernel comes from compiling csrc/twoview.hip once more with
-Rpass-analysis=kernel-resource-usage (no device needed).  There is no parent to compare with: the file states times, no bar."""
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
    """(kernel, VGPRs, scratch bytes per lane, static LDS bytes, occupancy in waves per SIMD) per kernel of twoview.hip"""
    from pram_amd import build
    src = build.CSRC / "twoview.hip"
    r = subprocess.run([build.HIPCC, *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", "/dev/null"],
                       capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"(twoview_\w+?_kernel|ransac_pick_kernel)", m.group(1))
            cur = {"name": name.group(1) if name else m.group(1)}
            rows.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("spill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def med(xs) -> str:
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def measure(n_pairs: int, trials: int, n_matches: int, reps: int) -> dict:
    import torch
    from pram_amd import ops
    from pram_amd.localization import triangulation as TG
    from pram_amd.localization import twoview as TV
    from tests import pose_ref as PR
    from tests import twoview_ref as TR
    dev = torch.device("cuda:0")
    cams = list(PR.SCENE_CAMERAS.values())
    sc = [TR.make_scene(5000 + i, cams[i % 5], cams[(i + 2) % 5], n_matches, 0.3) for i in range(n_pairs)]
    frames, cameras, pairs, matches = TR.batch(sc)
    table = TV.keypoint_table(frames, cameras, dev)
    use, pr, off, flat = TG._match_csr(table, pairs, matches)
    views = (table["norm05"], table["frame_off"], TG._up(pr, dev), TG._up(off, dev), TG._up(flat, dev))
    F, Pn, M = table["n_frames"], len(use), flat.shape[0]
    cam = (table["cam_model"], table["cam_params"])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    stage = {"hypotheses": [], "score": [], "finish": []}
    whole = []
    for rep in range(reps + 2):      # two warm-ups
        ev[0].record()
        h = ops.twoview_hypotheses(*views, F, Pn, M, trials=trials)
        ev[1].record()
        s = ops.twoview_score(*views, *cam, F, Pn, M, h["E"], h["n_sol"])
        ev[2].record()
        out = ops.twoview_finish(*views, *cam, F, Pn, M, h["E"], s["h_inliers"], s["best"])
        ev[3].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = TV.estimate_two_view(table, pairs, matches, trials=trials, pair_chunk=max(n_pairs, 1))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if rep >= 2:
            for k, (a, b) in zip(stage, ((0, 1), (1, 2), (2, 3))):
                stage[k].append(ev[a].elapsed_time(ev[b]))
            whole.append(dt)
    true = np.concatenate([~s_["outlier"] for s_ in sc])
    keep = np.concatenate(res["keep"])
    return {"stage": stage, "whole": whole, "success": int(res["success"].sum()), "recall": float(keep[true].mean()),
            "false": float(keep[~true].mean()), "workspace": n_pairs * trials * ops.TWOVIEW_TRIAL_BYTES, "out": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--trials", type=int, default=1024)
    ap.add_argument("--matches", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "twoview_timing.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("twoview_timing: no GPU (a time is measured on the device or not at all)")
    commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "working tree"
    lines = ["# Two-view estimator: time per stage", "",
             f"Measured {time.strftime('%Y-%m-%d')} on an MI355X by profiles/tools/twoview_timing.py, on top of commit {commit}.  Milliseconds, median "
             f"(smallest .. largest) of {a.reps} repetitions after two warm-ups; the stages between HIP events, the whole call (uploads, the three "
             "stages, one read-back) by a host clock around a device synchronise.  There is no parent to compare with and no bar.", ""]
    for n_pairs in (a.pairs, 1):
        m = measure(n_pairs, a.trials, a.matches, a.reps)
        tot = sum(statistics.median(v) for v in m["stage"].values())
        lines += [f"## {n_pairs} pair(s) x {a.trials} trials x {a.matches} matches", "",
                  "| stage | ms | share of the three |", "|---|---|---|"]
        for k, v in m["stage"].items():
            lines.append(f"| {k} | {med(v)} | {100.0 * statistics.median(v) / tot:.1f} % |")
        lines += [f"| estimate_two_view, whole call | {med(m['whole'])} | |", "",
                  f"Workspace of the chunk: {m['workspace'] / 2 ** 20:.1f} MiB.  {m['success']} of {n_pairs} pairs succeed; the masks keep "
                  f"{100.0 * m['recall']:.2f} % of the planted true matches and {100.0 * m['false']:.2f} % of the planted outliers.", ""]
        print("\n".join(lines[-9:]), flush=True)
    lines += ["## What the compiler reports (gfx950, -O3)", "", "| kernel | VGPRs | VGPR spills | scratch bytes / lane | static LDS bytes | occupancy (waves / SIMD) |",
              "|---|---|---|---|---|---|"]
    for r in resources():
        lines.append(f"| {r['name']} | {r.get('vgpr')} | {r.get('spill')} | {r.get('scratch')} | {r.get('lds')} | {r.get('occ')} |")
    lines += ["", "twoview_hypotheses_kernel also takes 141312 bytes of dynamic LDS per workgroup of one wave (276 doubles per lane), which the "
              "report does not count: one workgroup per CU, so the occupancy the LDS allows is one wave per CU.", ""]
    Path(a.out).write_text("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
