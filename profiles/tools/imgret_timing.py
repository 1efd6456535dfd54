"""Time of every stage of the image retrieval (pram_amd/localization/image_retrieval.py, csrc/imgret.hip) at production shapes;
writes profiles/imgret_timing.md.

    python profiles/tools/imgret_timing.py [--images 2000] [--rows 2048] [--k 64] [--reps 10] [--out FILE]

The descriptors: --images images of --rows unit rows each, scattered about 4 k random directions (what is timed does not depend on
the values beyond the labels' spread).  Every shape is warmed up twice; then --reps repetitions, each stage between two HIP events
on the current stream, and the whole calls by a host clock around work that ends in a device synchronise; medians with the
smallest and largest value.  Beside the two searches: torch.matmul + torch.topk on the same inputs, a point of comparison that
writes the queries x database matrix.  The compiler's resource report per kernel comes from compiling csrc/imgret.hip once more
with -Rpass-analysis=kernel-resource-usage (no device needed).  There is no parent to compare with: the file states times, no bar."""
from __future__ import annotations

import argparse
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def resources() -> list:
    from pram_amd import build
    src = build.CSRC / "imgret.hip"
    r = subprocess.run([build.HIPCC, *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", "/dev/null"],
                       capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"(imgret_\w+?_kernel)", m.group(1))
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


def timed(reps: int, fn) -> list:
    """fn between two HIP events, reps times after two warm-ups -> milliseconds."""
    import torch
    out = []
    for rep in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep >= 2:
            out.append(a.elapsed_time(b))
    return out


def walled(reps: int, fn) -> list:
    import torch
    out = []
    for rep in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= 2:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "imgret_timing.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("imgret_timing: no GPU (a time is measured on the device or not at all)")
    from pram_amd import ops
    from pram_amd.localization import image_retrieval as M
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    n_img, n_rows_img, k = a.images, a.rows, a.k
    n = n_img * n_rows_img
    dirs = torch.nn.functional.normalize(torch.randn(4 * k, 128, device=dev, generator=g), dim=1)
    x = torch.empty(n, 128, device=dev)
    for i in range(0, n, 1 << 20):      # built in slices: no second copy of the whole
        m = min(1 << 20, n - i)
        x[i:i + m] = torch.nn.functional.normalize(dirs[torch.randint(0, 4 * k, (m,), device=dev, generator=g)] + 0.08 * torch.randn(m, 128, device=dev, generator=g), dim=1)
    commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "working tree"
    lines = ["# Image retrieval: time per stage", "",
             f"Measured {time.strftime('%Y-%m-%d')} on an MI355X by profiles/tools/imgret_timing.py, on top of commit {commit}.  Milliseconds, median "
             f"(smallest .. largest) of {a.reps} repetitions after two warm-ups; the stages between HIP events, the whole calls by a host clock "
             "around a device synchronise.  There is no parent to compare with and no bar.", ""]

    # ---- the vocabulary: a sample of the rows
    sample = x[:: max(1, n // 262144)][:262144].contiguous()
    t_train = walled(max(2, a.reps // 3), lambda: M.train_vocabulary(sample, k=k, iters=20, seed=0, device=dev))
    vocab = M.train_vocabulary(sample, k=k, iters=20, seed=0, device=dev)
    lines += [f"## Vocabulary: {sample.shape[0]} rows, k = {k}, 20 iterations", "", "| call | ms |", "|---|---|",
              f"| train_vocabulary, whole call | {med(t_train)} |", ""]

    # ---- the global descriptors
    first = torch.arange(0, n, n_rows_img, device=dev, dtype=torch.int32)
    count = torch.full((n_img,), n_rows_img, device=dev, dtype=torch.int32)
    chunk = 1024
    labels, _ = ops.imgret_assign(x, vocab.centres)
    t_assign = timed(a.reps, lambda: ops.imgret_assign(x, vocab.centres))
    t_agg = timed(a.reps, lambda: [ops.imgret_aggregate(x, labels, vocab.centres, first[i:i + chunk], count[i:i + chunk]) for i in range(0, n_img, chunk)])
    sums = [ops.imgret_aggregate(x, labels, vocab.centres, first[i:i + chunk], count[i:i + chunk])[0] for i in range(0, n_img, chunk)]
    t_norm = timed(a.reps, lambda: [ops.imgret_normalize(s) for s in sums])
    del sums
    feats = {"descriptors": x.view(n_img, n_rows_img, 128), "counts": count}
    t_whole = walled(a.reps, lambda: M.global_descriptors(vocab, feats))
    vec = M.global_descriptors(vocab, feats)
    tot = sum(statistics.median(v) for v in (t_assign, t_agg, t_norm))
    lines += [f"## Global descriptors: {n_img} images x {n_rows_img} rows, k = {k} (image_chunk {chunk})", "", "| stage | ms | share of the three |", "|---|---|---|"]
    for name, v in (("assign", t_assign), ("aggregate", t_agg), ("normalize", t_norm)):
        lines.append(f"| {name} | {med(v)} | {100.0 * statistics.median(v) / tot:.1f} % |")
    lines += [f"| global_descriptors, whole call | {med(t_whole)} | |", "",
              f"assign is {n} x {k} x 128 squared differences in float64: {n * k * 128 * 3 / statistics.median(t_assign) / 1e9:.2f} T float64 operations / s "
              f"(a subtraction, a product and a sum each); it reads {n * 512 / 2 ** 30:.2f} GiB.", ""]
    print("\n".join(lines), flush=True)

    # ---- the searches
    L = k * 128
    big = torch.nn.functional.normalize(torch.randn(10000, L, device=dev, generator=g), dim=1)
    for title, q, db, excl in ((f"nq = nd = {n_img}, num_matched = 20, L = {L} (every image against the others)", vec, vec, torch.arange(n_img, device=dev, dtype=torch.int32)),
                               (f"nq = 16 against nd = 10000, num_matched = 20, L = {L}", big[:16].contiguous(), big, None)):
        nq, nd = q.shape[0], db.shape[0]
        sp = M.default_splits(nq, nd)
        rows = []
        for s in sorted({1, sp}):
            rows.append((f"pram_imgret_topk, splits = {s}" + (" (the default)" if s == sp else ""), timed(a.reps, lambda s=s: ops.imgret_topk(q, db, 20, excl, None, s))))
        rows.append(("retrieve, whole call", walled(a.reps, lambda: M.retrieve(q, db, 20, exclude=excl))))

        def torch_way():
            S = torch.matmul(q, db.T)
            if excl is not None:
                S[torch.arange(nq, device=dev), excl.long()] = -float("inf")
            return torch.topk(S, 20, dim=1)
        rows.append(("torch.matmul + torch.topk (writes the matrix)", timed(a.reps, torch_way)))
        ours = statistics.median(rows[-3][1])      # the row of the default splits
        lines += [f"## Search: {title}", "", "| call | ms |", "|---|---|"] + [f"| {nm} | {med(v)} |" for nm, v in rows]
        lines += ["", f"The products are {2.0 * nq * nd * L / 1e9:.1f} GFLOP: {2.0 * nq * nd * L / ours / 1e9:.1f} TFLOP/s at the default splits "
                  f"(queries are tiled by 32: {-(-nq // 32) * 32 * nd * L * 2.0 / ours / 1e9:.1f} TFLOP/s issued) against the 157 TFLOP/s fp32 peak.", ""]
        idx, _ = ops.imgret_topk(q, db, 20, excl, None, sp)
        _, ti = torch_way()
        agree = float((idx.long() == ti).float().mean())
        lines += [f"Lists against torch's on the same inputs: {100.0 * agree:.2f} % of the positions name the same index (the two round their sums differently).", ""]
        print("\n".join(lines[-12:]), flush=True)

    lines += ["## What the compiler reports (gfx950, -O3)", "", "| kernel | VGPRs | VGPR spills | scratch bytes / lane | static LDS bytes | occupancy (waves / SIMD) |",
              "|---|---|---|---|---|---|"]
    for r in resources():
        lines.append(f"| {r['name']} | {r.get('vgpr')} | {r.get('spill')} | {r.get('scratch')} | {r.get('lds')} | {r.get('occ')} |")
    lines += ["", f"imgret_assign_kernel also takes k x 512 bytes of dynamic LDS for the centres ({k * 512} at k = {k}, 131072 at 256), which the report "
              "does not count.", ""]
    Path(a.out).write_text("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
