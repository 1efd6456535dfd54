"""Time of cluster_points (pram_amd/localization/labelling.py, csrc/kmeans.hip) on the blob scene of tests/kmeans_ref.py at two sizes,
split into seeding, Lloyd iterations and read-backs, beside sklearn's KMeans(n_clusters=k, random_state=0) on the same points;
writes profiles/kmeans_timing.md.

    python profiles/tools/kmeans_timing.py [--sizes 200000:16,1500000:512] [--reps 5] [--threads 16] [--out FILE]
    python profiles/tools/kmeans_timing.py --sklearn-save FILE      # sklearn alone, on a machine without a GPU
    python profiles/tools/kmeans_timing.py --sklearn-load FILE      # use that record where sklearn does not import

Every size is warmed up once; then the repetitions of the sizes are interleaved (size A, size B, size A, ...), each timed by a host
clock around work that ends in a device synchronise; medians with the smallest and largest value.  The split needs a synchronise
after seeding and after the iterations, which an untimed run does not do; the whole call is also timed without the split.  Two
repetitions must give equal bits or nothing is written.  sklearn runs once per size (it is deterministic and takes long) on
--threads CPU threads.  Labels are compared with sklearn's as a finding, not as a gate."""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import kmeans_ref as KR  # noqa: E402

SEED = 31


def run_sklearn(sizes, threads):
    import sklearn
    from sklearn.cluster import KMeans
    try:
        from threadpoolctl import threadpool_limits
    except Exception:      # without it the thread count is the environment's
        threadpool_limits = None
    rec = {"version": sklearn.__version__, "threads": threads if threadpool_limits else "the environment's"}
    for n, k in sizes:
        xyz = KR.scene(n, k, SEED)
        t0 = time.perf_counter()
        if threadpool_limits:
            with threadpool_limits(limits=threads):
                m = KMeans(n_clusters=k, random_state=0).fit(xyz)
        else:
            m = KMeans(n_clusters=k, random_state=0).fit(xyz)
        rec[f"{n}:{k}"] = {"seconds": time.perf_counter() - t0, "n_iter": int(m.n_iter_), "labels": m.labels_.astype(np.int32), "inertia": float(m.inertia_)}
        print(f"sklearn {n} / {k}: {rec[f'{n}:{k}']['seconds']:.1f} s, {m.n_iter_} iterations", flush=True)
    return rec


def spread(v, unit=1e3):
    return f"{statistics.median(v) * unit:.1f} ({min(v) * unit:.1f} .. {max(v) * unit:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200000:16,1500000:512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kmeans_timing.md"))
    ap.add_argument("--sklearn-save")
    ap.add_argument("--sklearn-load")
    a = ap.parse_args()
    sizes = [tuple(int(x) for x in s.split(":")) for s in a.sizes.split(",")]
    if a.sklearn_save:
        rec = run_sklearn(sizes, a.threads)
        np.save(a.sklearn_save, rec, allow_pickle=True)
        return
    import torch
    from pram_amd.localization.labelling import cluster_points, ITER_GROUP
    assert torch.cuda.is_available(), "the timing needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    sk, sk_where = None, ""
    try:
        import sklearn  # noqa: F401
        sk, sk_where = run_sklearn(sizes, a.threads), f"the CPUs of the GPU host, {a.threads} threads"
    except ImportError:
        if a.sklearn_load:
            sk = np.load(a.sklearn_load, allow_pickle=True)[()]
            sk_where = f"NOT this machine: the development machine (no GPU), threads: {sk['threads']}"
    scenes = {s: KR.scene(s[0], s[1], SEED) for s in sizes}
    first = {}
    for s in sizes:      # warm-up, and the result every repetition has to equal
        first[s] = cluster_points(scenes[s], s[1], dev)
        print(f"warm {s}: {first[s]['n_iter']} iterations", flush=True)
    split = {s: {"prepare": [], "init": [], "lloyd": [], "readback": [], "total": []} for s in sizes}
    whole = {s: [] for s in sizes}
    reads = {}
    for r in range(a.reps):
        for s in sizes:
            t = {}
            t0 = time.perf_counter()
            got = cluster_points(scenes[s], s[1], dev, timings=t)
            split[s]["total"].append(time.perf_counter() - t0)
            for key in ("prepare", "init", "lloyd", "readback"):
                split[s][key].append(t[key])
            reads[s] = t["group_reads"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            again = cluster_points(scenes[s], s[1], dev)
            whole[s].append(time.perf_counter() - t0)
            for g in (got, again):
                assert np.array_equal(g["labels"], first[s]["labels"]) and np.array_equal(g["centers"].view(np.uint64), first[s]["centers"].view(np.uint64)) \
                    and g["n_iter"] == first[s]["n_iter"] and g["inertia"] == first[s]["inertia"], "two runs differ"
        print(f"repetition {r} done", flush=True)
    lines = ["# K-means labelling: cluster_points on the device beside sklearn", "",
             f"Written by `python profiles/tools/kmeans_timing.py --sizes {a.sizes} --reps {a.reps} --threads {a.threads}`.", "",
             f"Blob scene of tests/kmeans_ref.py (sigma 6 around k centres in +-50 m, seed {SEED}), mode 'xyz', tol 1e-4, max_iter 300, k-means++ with",
             f"seed 0.  Times in ms: median of {a.reps} interleaved repetitions (min .. max), host clock around work that ends in a device",
             "synchronise, after one warm-up per size.  Every repetition gave the same bits as the warm-up.", ""]
    for s in sizes:
        n, k = s
        it = first[s]["n_iter"]
        lines += [f"## {n} points, k = {k}", "", "| | |", "|---|---|",
                  f"| iterations / relocations / inertia | {it} / {first[s]['relocations']} / {first[s]['inertia']:.6e} |",
                  f"| whole call, no split | {spread(whole[s])} |",
                  f"| whole call with the split's synchronises | {spread(split[s]['total'])} |",
                  f"| host preparation in numpy (finite check, mask, mean, centring, variance) | {spread(split[s]['prepare'])} |",
                  f"| upload and k-means++ seeding ({3 * (k - 1) + 4} launches) | {spread(split[s]['init'])} |",
                  f"| Lloyd iterations and the finish ({4 * it} + 4 launches, up to {ITER_GROUP - 1} more iterations enqueued that return at once) | {spread(split[s]['lloyd'])} |",
                  f"| per iteration (Lloyd time / iterations) | {statistics.median(split[s]['lloyd']) / it * 1e3:.3f} |",
                  f"| read-backs: {reads[s]} of the done word (groups of {ITER_GROUP}), then labels, centres and state | {spread(split[s]['readback'])} |"]
        key = f"{n}:{k}"
        if sk is not None and key in sk:
            differ = int((sk[key]["labels"] != first[s]["labels"]).sum())
            lines += [f"| sklearn {sk['version']} KMeans(random_state=0), one run ({sk_where}) | {sk[key]['seconds']:.2f} s, {sk[key]['n_iter']} iterations |",
                      f"| labels that differ from sklearn's | {differ} of {n} |",
                      f"| inertia: sklearn / device | {sk[key]['inertia']:.6e} / {first[s]['inertia']:.6e} |"]
        else:
            lines += ["| sklearn | not measured: it does not import on the GPU host and no record was given |"]
        lines += [""]
    lines += ["Not measured: per-kernel times (no profiler run), so how an iteration divides between the assignment, the cluster sums, the",
              "reduction of the block partials and the single-workgroup update is not known, nor how the seeding figure divides between the",
              "upload, the host's random numbers and its launches; any k above 512; the relocation path on a large input.", ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
