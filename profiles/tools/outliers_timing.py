"""Time of statistical_inliers (pram_amd/localization/outliers.py, csrc/knn.hip) on clustered random points at three sizes, split
into upload, the k-NN kernel, the selection and the read-back, beside scipy's cKDTree.query on the same points and the same box;
writes profiles/outliers_timing.md.

    python profiles/tools/outliers_timing.py [--sizes 100000,1000000,2000000] [--k 20] [--reps 5] [--threads 16] [--out FILE]

Every size is warmed up once; then the repetitions of the sizes are interleaved (size A, size B, size A, ...), each timed by a host
clock around work that ends in a device synchronise; medians with the smallest and largest value.  The split needs a synchronise
after every stage, which an untimed run does not do; the whole call is also timed without the split.  Every repetition must give
the warm-up's bits or nothing is written.  The k-d tree (build and query, --threads workers) runs once per size: its mask is
compared with the device's as a finding, not as a gate."""
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

SEED = 41


def points(n: int) -> np.ndarray:
    """One cluster per 2000 points (sigma 4) with centres in +-300 m, and one point in 200 uniform over the box: a map's order of
    density, not its shape."""
    rs = np.random.RandomState(SEED)
    c = max(n // 2000, 1)
    centres = rs.uniform(-300.0, 300.0, size=(c, 3))
    x = centres[rs.randint(0, c, size=n)] + rs.normal(0.0, 4.0, size=(n, 3))
    stray = rs.uniform(size=n) < 0.005
    x[stray] = rs.uniform(-400.0, 400.0, size=(int(stray.sum()), 3))
    return np.ascontiguousarray(x)


def kd_tree(x: np.ndarray, k: int, ratio: float, threads: int) -> dict:
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(x)
    t1 = time.perf_counter()
    d, _ = tree.query(x, k, workers=threads)
    t2 = time.perf_counter()
    avg = d.mean(axis=1)
    v = avg > 0
    th = avg[v].mean() + ratio * avg[v].std(ddof=1)
    return {"build": t1 - t0, "query": t2 - t1, "mask": v & (avg < th), "avg": avg}


def spread(v, unit=1e3):
    return f"{statistics.median(v) * unit:.1f} ({min(v) * unit:.1f} .. {max(v) * unit:.1f})"


def resource_usage() -> list:
    """VGPRs and scratch of every instance of the k-NN kernel, from the compiler's own remarks."""
    from pram_amd import build
    src = build.CSRC / "knn.hip"
    r = subprocess.run([build.HIPCC, *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", "/dev/null"],
                       capture_output=True, text=True)
    rows, name = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name and "knn_mean_distance_kernel" in name:
            rows.append((re.search(r"ILi(\d+)E", name).group(1), m.group(1), int(m.group(2))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,2000000")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "outliers_timing.md"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    import torch
    from pram_amd.localization.outliers import statistical_inliers
    assert torch.cuda.is_available(), "the timing needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    scenes = {n: points(n) for n in sizes}
    first = {}
    for n in sizes:      # warm-up, and the result every repetition has to equal
        first[n] = statistical_inliers(scenes[n], dev, a.k, a.ratio)
        print(f"warm {n}: {len(first[n]['inlier_ids'])} inliers of {first[n]['n_valid']} valid", flush=True)
    keys = ("upload", "knn", "select", "readback")
    split = {n: {key: [] for key in keys + ("total",)} for n in sizes}
    whole = {n: [] for n in sizes}
    for r in range(a.reps):
        for n in sizes:
            t = {}
            t0 = time.perf_counter()
            got = statistical_inliers(scenes[n], dev, a.k, a.ratio, timings=t)
            split[n]["total"].append(time.perf_counter() - t0)
            for key in keys:
                split[n][key].append(t[key])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            again = statistical_inliers(scenes[n], dev, a.k, a.ratio)
            whole[n].append(time.perf_counter() - t0)
            for g in (got, again):
                assert all(np.asarray(g[key]).tobytes() == np.asarray(first[n][key]).tobytes() for key in g), "two runs differ"
        print(f"repetition {r} done", flush=True)
    kd = {}
    for n in sizes:
        kd[n] = kd_tree(scenes[n], a.k, a.ratio, a.threads)
        print(f"k-d tree {n}: build {kd[n]['build']:.2f} s, query {kd[n]['query']:.2f} s", flush=True)
    lines = ["# Statistical outlier removal: statistical_inliers on the device beside a k-d tree", "",
             f"Written by `python profiles/tools/outliers_timing.py --sizes {a.sizes} --k {a.k} --reps {a.reps} --threads {a.threads}`.", "",
             f"Clustered random points (one cluster of sigma 4 per 2000 points, centres in +-300 m, 0.5 % strays; seed {SEED}), nb_neighbors {a.k},",
             f"std_ratio {a.ratio}.  Times in ms: median of {a.reps} interleaved repetitions (min .. max), host clock around work that ends in a",
             "device synchronise, after one warm-up per size.  Every repetition gave the same bits as the warm-up.  A pair evaluation is one",
             "candidate against one query: three differences, three products, two sums and one comparison in float64.", ""]
    for n in sizes:
        knn = statistics.median(split[n]["knn"])
        lines += [f"## {n} points", "", "| | |", "|---|---|",
                  f"| valid / inliers / threshold | {first[n]['n_valid']} / {len(first[n]['inlier_ids'])} / {first[n]['threshold']:.6f} |",
                  f"| whole call, no split | {spread(whole[n])} |",
                  f"| whole call with the split's synchronises | {spread(split[n]['total'])} |",
                  f"| host check (shape, finite) and upload | {spread(split[n]['upload'])} |",
                  f"| k-NN kernel (pram_knn_mean_distance, one launch) | {spread(split[n]['knn'])} |",
                  f"| pair evaluations per second ({n}^2 / the kernel's median) | {n * n / knn:.3e} |",
                  f"| selection (pram_sor_select, seven launches) | {spread(split[n]['select'])} |",
                  f"| read-back (counts, statistics, indices, mask, avg) | {spread(split[n]['readback'])} |",
                  f"| scipy cKDTree on the CPUs of the same box: build, then query(k = {a.k}, workers = {a.threads}), one run | {kd[n]['build']:.2f} s + {kd[n]['query']:.2f} s |",
                  f"| mask entries that differ from the k-d tree's / largest difference in avg | {int((kd[n]['mask'] != first[n]['mask']).sum())} of {n} / {np.abs(kd[n]['avg'] - first[n]['avg_distance']).max():.2e} |",
                  ""]
    lines += ["## The k-NN kernel's registers", "",
              "`-Rpass-analysis=kernel-resource-usage` on csrc/knn.hip with the library's flags; one instance per list size (the entry takes",
              "the smallest that holds min(k, n)).", "", "| list slots | VGPRs | scratch bytes / lane | waves / SIMD | LDS bytes / block |", "|---|---|---|---|---|"]
    try:
        rows = resource_usage()
        for ks in sorted({r[0] for r in rows}, key=int):
            v = {name: val for s, name, val in rows if s == ks}
            lines += [f"| {ks} | {v.get('VGPRs')} | {v.get('ScratchSize [bytes/lane]')} | {v.get('Occupancy [waves/SIMD]')} | {v.get('LDS Size [bytes/block]')} |"]
    except Exception as e:      # no compiler on this machine
        lines += [f"| not measured: {e} | | | | |"]
    lines += ["", "Not measured: the kernel under a profiler (how its time divides between the distance arithmetic, the LDS reads and the",
              "insertions is not known); points in a real map's order, where neighbours in space are neighbours in index and a list warms up",
              "differently; nb_neighbors other than the one above.", ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
