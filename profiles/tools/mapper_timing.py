"""Time of every stage of the incremental mapper (pram_amd/localization/mapper.py, csrc/mapper.hip) on a simulated street, and
the rounds it ran; writes profiles/mapper_timing.md.

    python profiles/tools/mapper_timing.py [--frames 120] [--points 6000] [--out FILE]

The street: --frames pinhole cameras (640 x 480, f = 500) half a metre apart, looking sideways and turned a little from frame to
frame; --points points 4 to 12 m away, each seen by about 60 % of the frames that have it in view, 0.5 px noise; matches between
frames at most three apart, one wrong match in ten.  No poses go in.  One warm-up call, then one timed call: every stage function
of the module is wrapped by a host clock between two device synchronisations, so the stages add up to a little more than an
unwrapped call, which is timed as well.  The compiler's resource report per kernel comes from compiling csrc/mapper.hip once more
with -Rpass-analysis=kernel-resource-usage (no device needed).  There is no parent to compare with and no bar: the file states
one run's times.  Nothing else about this stage's speed has been measured."""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import time
from collections import defaultdict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def resources() -> list:
    """(kernel, VGPRs, scratch bytes per lane, static LDS bytes, occupancy in waves per SIMD) per kernel of mapper.hip"""
    from pram_amd import build
    src = build.CSRC / "mapper.hip"
    r = subprocess.run([build.HIPCC, *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", "/dev/null"],
                       capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"(map_\w+?_kernel)(ILb(\d)E)?", m.group(1))
            cur = {"name": (name.group(1) + ("<fill>" if name.group(3) == "1" else "<count>" if name.group(3) == "0" else "")) if name else m.group(1)}
            rows.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return [r for r in rows if r["name"].startswith("map_")]


def simulate(n_frames: int, n_points: int, seed: int = 0) -> dict:
    """-> frames, cameras, pairs, matches and the true centres, all by numpy."""
    from tests import pose_ref as PR
    rng = np.random.RandomState(seed)
    step, f0, w, h = 0.5, 500.0, 640, 480
    cx = np.arange(n_frames) * step
    yaw = np.deg2rad(3.0) * np.sin(np.arange(n_frames) * 0.3)
    Rs = [PR.rodrigues(np.array([0.0, a, 0.0])) for a in yaw]
    C = np.stack([cx, 0.05 * np.sin(np.arange(n_frames) * 0.5), np.zeros(n_frames)], 1)
    X = np.stack([rng.uniform(-3.0, cx[-1] + 3.0, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(4.0, 12.0, n_points)], 1)
    kps, where = [], []
    for f in range(n_frames):
        Y = (X - C[f]) @ Rs[f].T
        u, v = f0 * Y[:, 0] / Y[:, 2] + w / 2, f0 * Y[:, 1] / Y[:, 2] + h / 2
        see = np.nonzero((Y[:, 2] > 0.5) & (u >= 8) & (u < w - 8) & (v >= 8) & (v < h - 8) & (rng.uniform(size=n_points) < 0.6))[0]
        see = see[rng.permutation(len(see))]
        kps.append((np.stack([u[see], v[see]], 1) - 0.5 + rng.normal(size=(len(see), 2)) * 0.5).astype(np.float32))
        idx = np.full(n_points, -1, dtype=np.int64)
        idx[see] = np.arange(len(see))
        where.append(idx)
    pairs, matches = [], []
    for a in range(n_frames):
        for b in range(a + 1, min(a + 4, n_frames)):
            both = np.nonzero((where[a] >= 0) & (where[b] >= 0))[0]
            m = np.stack([where[a][both], where[b][both]], 1)
            k = len(m) // 9
            wrong = np.stack([rng.randint(0, len(kps[a]), k), rng.randint(0, len(kps[b]), k)], 1)
            pairs.append((a, b)); matches.append(np.concatenate([m, wrong])[rng.permutation(len(m) + k)])
    return {"frames": [{"keypoints": k} for k in kps], "cameras": [("SIMPLE_PINHOLE", w, h, [f0, w / 2.0, h / 2.0])] * n_frames, "pairs": pairs,
            "matches": matches, "centres": C, "n_matches": int(sum(len(m) for m in matches)), "n_keypoints": int(sum(len(k) for k in kps))}


def measure(sim: dict) -> dict:
    import torch
    from pram_amd import ops
    from pram_amd.localization import bundle, mapper, pose, triangulation, twoview
    dev = torch.device("cuda:0")
    args = (sim["frames"], sim["cameras"], sim["pairs"], sim["matches"], dev)
    mapper.reconstruct(*args)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = mapper.reconstruct(*args)
    torch.cuda.synchronize()
    whole = (time.perf_counter() - t0) * 1e3
    times, calls = defaultdict(float), defaultdict(int)

    def wrap(owner, name, label):
        fn = getattr(owner, name)

        def timed(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            times[label] += (time.perf_counter() - t) * 1e3
            calls[label] += 1
            return out
        setattr(owner, name, timed)
        return lambda: setattr(owner, name, fn)

    undo = [wrap(twoview, "keypoint_table", "frame table (uploads, normalised keypoints)"), wrap(twoview, "_estimate", "stage 0: two-view geometry of every pair"),
            wrap(ops, "tri_adjacency", "stage 0: adjacency"), wrap(mapper, "_scores", "stage 1: pram_map_pair_angles"),
            wrap(mapper, "_seed", "stage 1: pram_map_seed and its read-back"), wrap(ops, "map_correspond", "stage 3: pram_map_correspond"),
            wrap(ops, "map_choose", "stage 4: pram_map_choose"), wrap(ops, "map_pack", "stage 4: pram_map_pack"),
            wrap(pose, "estimate_poses", "stage 4: pose.estimate_poses"), wrap(mapper, "_triangulate", "stage 5: live edges, tracks, triangulation"),
            wrap(mapper, "_adjust", "stage 5: observation tables and bundle adjustment"), wrap(mapper, "_verified", "the end: the matches against the final poses"), wrap(triangulation, "_tables", "the end: the host's tables"),
            wrap(bundle, "bundle_adjust", "the end: bundle_adjust")]
    t0 = time.perf_counter()
    again = mapper.reconstruct(*args)
    torch.cuda.synchronize()
    wrapped = (time.perf_counter() - t0) * 1e3
    for u in undo:
        u()
    assert np.array_equal(again["registered"], res["registered"])
    reg = np.nonzero(res["registered"])[0]
    err = float("nan")
    if len(reg) >= 3:
        s, R, t = mapper.similarity_from_centres(mapper.centres(res["qvecs"], res["tvecs"])[reg], sim["centres"][reg])
        moved = mapper.apply_similarity(res, s, R, t)
        err = float(np.linalg.norm(mapper.centres(moved["qvecs"], moved["tvecs"])[reg] - sim["centres"][reg], axis=1).max())
    return {"whole": whole, "wrapped": wrapped, "times": dict(times), "calls": dict(calls), "res": res, "centre_error": err,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mapper_timing.md"))
    a = ap.parse_args()
    sim = simulate(a.frames, a.points)
    m = measure(sim)
    res, rep = m["res"], m["res"]["report"]
    out = ["# Incremental mapper: one timed run", "",
           f"Written by `profiles/tools/mapper_timing.py --frames {a.frames} --points {a.points}` on {m['device']}.  One run after one warm-up; no bar is set",
           "and nothing else about this stage's speed has been measured.", "",
           f"The street: {a.frames} frames, {sim['n_keypoints']} keypoints, {len(sim['pairs'])} pairs, {sim['n_matches']} matches (one in ten wrong), no poses.",
           f"Result: {int(res['registered'].sum())} of {a.frames} frames registered in {len(rep['rounds']) - 1} rounds after the seed "
           f"(seed frames {rep['seed_frames']}, thresholds halved {rep['seed_relaxed']} times), {len(res['point_ids'])} points; largest centre error after the",
           f"alignment to the true centres {m['centre_error']:.4f} m.", "",
           f"The whole call: **{m['whole']:.1f} ms**; with every stage between two synchronisations {m['wrapped']:.1f} ms, split as follows.", "",
           "| stage | calls | ms | share |", "|---|---:|---:|---:|"]
    total = sum(m["times"].values())
    for k, v in m["times"].items():
        out.append(f"| {k} | {m['calls'][k]} | {v:.1f} | {100 * v / total:.1f} % |")
    out += [f"| (host code between the stages) | | {m['wrapped'] - total:.1f} | |", "", "## The rounds", "",
            "| round | frames tried | accepted | points | observations | BA end | BA cost |", "|---:|---:|---:|---:|---:|---|---:|"]
    for i, r in enumerate(rep["rounds"]):
        out.append(f"| {i} | {len(r['frames_tried'])} | {len(r['frames_accepted'])} | {r['points']} | {r['observations']} | {r['ba_termination']} ({r['ba_iterations']}) | {r['ba_final_cost']:.1f} |")
    out += ["", "## The kernels of mapper.hip (compiler's report)", "", "| kernel | VGPRs | scratch B/lane | LDS B | waves/SIMD |", "|---|---:|---:|---:|---:|"]
    for r in resources():
        out.append(f"| `{r['name']}` | {r.get('vgpr')} | {r.get('scratch')} | {r.get('lds')} | {r.get('occ')} |")
    Path(a.out).write_text("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
