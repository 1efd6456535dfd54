"""Time of every stage of triangulate_map (pram_amd/localization/triangulation.py, csrc/triangulate.hip) on a synthetic scene of a
production shape, without wrong matches and with 2 % of them, with and without stage 2b (min_support), beside the parent commit's
triangulate_map on the same inputs; writes profiles/triangulation_timing.md.

    python profiles/tools/triangulation_timing.py [--frames 1000] [--keypoints 2048] [--reps 5] [--parent FILE] [--out FILE]

The scene: --frames cameras on a closed ring, every frame with --keypoints keypoints, every point seen in 32 consecutive frames,
pairs (f, f + 1 .. f + 20), a shared point matched with the probability that gives 300 matches per pair on average.  A wrong match
joins a keypoint to the keypoint of another point that lies nearest to its epipolar line (below 3 px, so it passes verification).
Each scene is warmed up once; then the repetitions of all runs are interleaved, each timed by a host clock around work that ends in
a device synchronise; medians with the smallest and largest value.  The split synchronises after every stage, which the whole call
does not.  --parent: the parent commit's triangulation.py (git show HEAD~:pram_amd/localization/triangulation.py > FILE), loaded
beside the current one on the same library; without it that column is left out.  The host side runs on 16 CPU threads at most."""
from __future__ import annotations

import argparse
import importlib.util
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
for _k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
    os.environ[_k] = str(min(int(os.environ.get(_k, 16)), 16))

SEED, SEEN, SPAN, PER_PAIR, NOISE = 17, 32, 20, 300, 0.4


def scene(F: int, K: int, p: float) -> dict:
    from tests import triangulation_ref as TR
    rng = np.random.RandomState(SEED)
    J = K // SEEN                       # points whose first frame is f, for every f
    assert J * SEEN == K and F > 2 * SEEN
    ang = np.linspace(0.0, 2.0 * np.pi, F, endpoint=False)
    centres = [np.array([9.0 * np.sin(a), 0.4 * np.sin(5 * a), -9.0 * np.cos(a)]) for a in ang]
    s = TR._base([TR.CAMERAS[f % 5] for f in range(F)], centres, [np.zeros(3)] * F)
    xyz = rng.uniform(-1.0, 1.0, size=(F * J, 3))
    # frame f's keypoint i * J + j is point ((f - i) mod F) * J + j: the point that started i frames ago
    pid = (((np.arange(F)[:, None, None] - np.arange(SEEN)[None, :, None]) % F) * J + np.arange(J)[None, None, :]).reshape(F, K)
    kp = np.stack([TR.project(s, f, xyz[pid[f]])[0] for f in range(F)]) - 0.5 + rng.uniform(-NOISE, NOISE, size=(F, K, 2))
    kp = kp.astype(np.float32)
    shared = sum((SEEN - d) * J for d in range(1, SPAN + 1))
    q = PER_PAIR * SPAN / shared
    pairs, matches = [], []
    for d in range(1, SPAN + 1):
        i, j = (x.ravel() for x in np.meshgrid(np.arange(SEEN - d), np.arange(J), indexing="ij"))
        m = np.stack([i * J + j, (i + d) * J + j], 1)
        take = rng.uniform(size=(F, len(m))) < q
        for f in range(F):
            pairs.append((f, (f + d) % F))
            matches.append(m[take[f]])
    n_true, n_wrong = sum(len(m) for m in matches), 0
    if p > 0:
        norm0 = np.stack([TR.normalize(kp[f], [0, K], s["cam_model"][f:f + 1], s["cam_params"][f:f + 1], 0.0) for f in range(F)])
        for k, (a, b) in enumerate(pairs):
            n = int(rng.binomial(len(matches[k]), p))
            if n == 0:
                continue
            i = rng.randint(K, size=n)
            e0, e1 = TR.epipolar_errors(TR.essential(s["table"][a], s["table"][b]), np.repeat(norm0[a][i], K, axis=0), np.tile(norm0[b], (n, 1)))
            cost = np.maximum(e0 * s["table"][a, 15], e1 * s["table"][b, 15]).reshape(n, K)
            cost[pid[a][i][:, None] == pid[b][None, :]] = np.inf
            j = cost.argmin(1)
            ok = cost[np.arange(n), j] < 3.0
            matches[k] = np.concatenate([matches[k], np.stack([i[ok], j[ok]], 1)])
            n_wrong += int(ok.sum())
    s.update(frames=[{"keypoints": kp[f]} for f in range(F)], pairs=np.array(pairs), matches=matches, n_true=n_true, n_wrong=n_wrong, p=p)
    return s


def split(TG, ops, torch, s, dev, ms: int) -> dict:
    """triangulate_map's body with a synchronise and a clock after every stage."""
    p = {**TG.DEFAULTS, "min_support": ms}
    t, t0 = {}, time.perf_counter()

    def lap(name):
        nonlocal t0
        torch.cuda.synchronize()
        now = time.perf_counter()
        t[name], t0 = now - t0, now

    table = TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), dev)
    lap("1 frame table, normalised keypoints (with the upload)")
    v = TG._verify(table, s["pairs"], s["matches"], p["max_error"])
    lap("2 verification (with the matches' upload)")
    edges = v["edges"]
    if ms:
        a = ops.tri_adjacency(edges, v["n_matches"], table["frame_off"], table["n_frames"], table["n_rows"])
        lap("2b adjacency")
        edges = ops.tri_support(table["norm05"], table["keypoints"], table["frames"], table["cam_model"], table["cam_params"], edges, v["n_matches"],
                                a["adj_off"], a["adj"], a["row_frame"], table["n_frames"], table["n_rows"], float(np.deg2rad(p["min_tri_angle"])),
                                p["max_reproj_error"], ms)["edges"]
        lap("2b support")
    trk = TG._tracks(table, edges, v["n_matches"])
    lap("3 components and tracks")
    out = TG._triangulate(table, trk, p)
    lap("4 triangulation")
    sizes = np.diff(trk["trk_off"][:trk["n_tracks"] + 1].cpu().numpy())
    t["_tracks"], t["_largest"], t["_accepted"] = trk["n_tracks"], int(sizes.max(initial=0)), int(out["accept"][:trk["n_tracks"]].sum().item())
    return t


def spread(v, unit=1e3):
    return f"{statistics.median(v) * unit:.1f} ({min(v) * unit:.1f} .. {max(v) * unit:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--keypoints", type=int, default=2048)
    ap.add_argument("--shares", default="0,0.02")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulation_timing.md"))
    a = ap.parse_args()
    import torch
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    from pram_amd import ops
    from pram_amd.localization import triangulation as TG
    assert torch.cuda.is_available(), "the timing needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    parent = None
    if a.parent:
        spec = importlib.util.spec_from_file_location("parent_triangulation", a.parent)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
    shares = [float(x) for x in a.shares.split(",")]
    scenes = {}
    for p in shares:
        t0 = time.perf_counter()
        scenes[p] = scene(a.frames, a.keypoints, p)
        print(f"scene p = {p}: {scenes[p]['n_true']} true and {scenes[p]['n_wrong']} wrong matches over {len(scenes[p]['pairs'])} pairs, built in {time.perf_counter() - t0:.1f} s", flush=True)
    call = lambda mod, s, **kw: mod.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev, **kw)
    runs = [(p, name) for p in shares for name in (("parent",) if parent else ()) + ("min_support 0", "min_support 1")]
    do = {"parent": lambda s: call(parent, s), "min_support 0": lambda s: call(TG, s), "min_support 1": lambda s: call(TG, s, min_support=1)}
    first, whole, stages = {}, {r: [] for r in runs}, {r: [] for r in runs if r[1] != "parent"}
    for r in runs:      # warm-up, and the result every repetition has to equal
        t0 = time.perf_counter()
        first[r] = do[r[1]](scenes[r[0]])
        print(f"warm {r}: {len(first[r]['point_ids'])} points in {time.perf_counter() - t0:.2f} s", flush=True)
    for p in shares:
        if parent:
            assert all(np.array_equal(first[(p, "parent")][k], first[(p, "min_support 0")][k]) for k in ("point_ids", "point3D_xyzs", "track_error")), "min_support 0 is not the parent"
    for rep in range(a.reps):
        for r in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = do[r[1]](scenes[r[0]])
            whole[r].append(time.perf_counter() - t0)
            assert np.array_equal(got["point3D_xyzs"], first[r]["point3D_xyzs"]), "two runs differ"
            if r in stages:
                stages[r].append(split(TG, ops, torch, scenes[r[0]], dev, int(r[1][-1])))
        print(f"repetition {rep} done", flush=True)
    F, K = a.frames, a.keypoints
    lines = ["# Triangulation: the time of every stage of triangulate_map", "",
             f"Written by `python profiles/tools/triangulation_timing.py --frames {F} --keypoints {K} --shares {a.shares} --reps {a.reps}" + (" --parent FILE`." if parent else "`."), "",
             f"A synthetic scene of a production shape: {F} frames on a closed ring, {K} keypoints each ({F * K} rows), every point seen in {SEEN}",
             f"consecutive frames, {SPAN} pairs per frame ({F * SPAN} pairs), {PER_PAIR} matches per pair on average, keypoint noise +-{NOISE} px; seed {SEED}.",
             "A wrong match joins a keypoint to the keypoint of another point nearest to its epipolar line and passes verification.  Times in",
             f"ms: median of {a.reps} interleaved repetitions (min .. max), host clock around work that ends in a device synchronise, after one",
             "warm-up per run.  Every repetition gave the warm-up's points bit for bit" + (", and min_support 0 gave the parent's." if parent else "."), ""]
    for p in shares:
        s = scenes[p]
        lines += [f"## Wrong matches: {p * 100:g} % ({s['n_true']} true, {s['n_wrong']} wrong)", "", "| | " + " | ".join(n for q, n in runs if q == p) + " |",
                  "|---|" + "---|" * sum(1 for q, n in runs if q == p)]
        cols = [r for r in runs if r[0] == p]
        lines += ["| whole call, no split | " + " | ".join(spread(whole[r]) for r in cols) + " |"]
        lines += ["| points | " + " | ".join(str(len(first[r]["point_ids"])) for r in cols) + " |"]
        for key in ("_tracks", "_largest", "_accepted"):
            lines += [f"| {dict(_tracks='tracks', _largest='largest track (rows)', _accepted='accepted tracks')[key]} | " +
                      " | ".join(str(stages[r][0][key]) if r in stages else "" for r in cols) + " |"]
        names = sorted({k for r in cols if r in stages for k in stages[r][0] if not k.startswith("_")})
        for k in names:
            lines += [f"| {k} | " + " | ".join(spread([t[k] for t in stages[r]]) if r in stages and k in stages[r][0] else "" for r in cols) + " |"]
        lines += ["| the split's stages together | " + " | ".join(spread([sum(v for k, v in t.items() if not k.startswith("_")) for t in stages[r]]) if r in stages else "" for r in cols) + " |", ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    old = Path(a.out).read_text() if Path(a.out).exists() else ""
    if "## Reading" in old:      # written by hand below the tables: carried over, to be read again against the new numbers
        lines += [old[old.index("## Reading"):]]
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
