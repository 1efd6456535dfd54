"""Time of compress_map's selection (csrc/compress.hip) on a map-like size, beside the numpy restatement of the reference
(tests/compress_ref.py) on the same inputs, and the share of the device time that is launch overhead; writes
profiles/compress_timing.md.

    python profiles/tools/compress_timing.py [--frames 2000] [--rows 2000] [--vrfs 256] [--covisible 30] [--threads 16] [--out FILE]

The synthetic map: a camera moving along x past a strip of points, every frame observing --rows of the points it sees (keypoint =
projection + noise); every --frames / --vrfs-th frame is a reference frame.  The restatement runs first, with the distance step in
torch on --threads CPU threads (the reference builds the same matrix in torch) and rows already discarded not measured again.
The device side is timed between HIP events, warm, workspace allocated beforehand.  Launch overhead: the same sequence of
launches on a map of the same frames and lists whose frames have one row with id -1 each, so that no kernel has work.  The two
sides' results are compared before any figure is written."""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import compress_ref as CR  # noqa: E402


def make_map(n_frames, n_rows, seed=11):
    rng = np.random.default_rng(seed)
    step, depth = 0.2, (5.0, 8.0)
    length = step * n_frames + 10.0
    n_points = int(1.6 * n_rows * length / 8.0)
    xyz = np.stack([rng.uniform(-5.0, length - 5.0, n_points), rng.uniform(-2.2, 2.2, n_points), rng.uniform(*depth, n_points)], axis=1)
    order = np.argsort(xyz[:, 0])
    xyz = xyz[order]
    cams = np.zeros((n_frames, 13))
    cams[:, 0], cams[:, 7:11], cams[:, 11], cams[:, 12] = 1.0, CR.INTRINSICS, CR.WIDTH, CR.HEIGHT
    cams[:, 4] = -step * np.arange(n_frames)
    ids, xys, frame_off = [], [], [0]
    for f in range(n_frames):
        lo, hi = np.searchsorted(xyz[:, 0], [step * f - 5.5, step * f + 5.5])
        u, v, Z = CR.project(cams[f], xyz[lo:hi])
        vis = np.nonzero((u > 1) & (u < CR.WIDTH - 1) & (v > 1) & (v < CR.HEIGHT - 1))[0]
        pick = np.sort(rng.choice(vis, size=min(n_rows, len(vis)), replace=False))
        ids.append(lo + pick + 1)
        xys.append(np.stack([u[pick], v[pick]], axis=1) + 0.7 * rng.standard_normal((len(pick), 2)))
        frame_off.append(frame_off[-1] + len(pick))
    row_ids = np.concatenate(ids).astype(np.int64)
    frame_off = np.array(frame_off, dtype=np.int32)
    row_frame = np.repeat(np.arange(n_frames), np.diff(frame_off))
    by_point = np.argsort(row_ids, kind="stable")
    pt_ids, counts = np.unique(row_ids, return_counts=True)
    pt_off = np.zeros(len(pt_ids) + 1, dtype=np.int64)
    pt_off[1:] = np.cumsum(counts)
    return dict(frame_off=frame_off, row_ids=row_ids, xys=np.concatenate(xys), cams=cams, pt_ids=pt_ids, pt_xyz=xyz[pt_ids - 1], pt_off=pt_off,
                pt_frames=row_frame[by_point].astype(np.int32), n_frames=n_frames)


def covisible(m, vrf, n):
    """The store's graph for the reference frames: count descending, frame index ascending, cut at n."""
    off = np.zeros(m["n_frames"] + 1, dtype=np.int32)
    lists = {}
    for v in vrf:
        at = np.searchsorted(m["pt_ids"], m["row_ids"][m["frame_off"][v]:m["frame_off"][v + 1]])
        cnt = np.bincount(np.concatenate([m["pt_frames"][m["pt_off"][p]:m["pt_off"][p + 1]] for p in at]), minlength=m["n_frames"])
        fr = np.nonzero(cnt)[0]
        lists[v] = fr[np.lexsort((fr, -cnt[fr]))][:n].tolist()
    for f in range(m["n_frames"]):
        off[f + 1] = off[f] + len(lists.get(f, []))
    return lists, off, np.array([c for f in sorted(lists) for c in lists[f]], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--vrfs", type=int, default=256)
    ap.add_argument("--covisible", type=int, default=30)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=float, default=20.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "compress_timing.md"))
    a = ap.parse_args()
    import torch
    torch.set_num_threads(a.threads)
    t0 = time.time()
    m = make_map(a.frames, a.rows)
    vrf = [int(x) for x in np.linspace(0, a.frames - 1, a.vrfs).round().astype(int)]
    lists, covis_off, covis_frames = covisible(m, sorted(set(vrf)), a.covisible)
    n_rows = int(m["frame_off"][-1])
    steps = sum(sum(1 for c in lists[v] if c != v) for v in vrf)
    launches = 2 + len(vrf) + 2 * steps
    print(f"map made in {time.time() - t0:.1f} s: {a.frames} frames, {n_rows} rows, {len(m['pt_ids'])} points, {len(vrf)} reference frames, "
          f"{steps} steps, {launches} launches", flush=True)

    # ---- the restatement, before the device is touched
    calls = [0]

    def min_dist(u, w, kp):
        calls[0] += 1
        if calls[0] % 2000 == 0:
            print(f"  restatement: {calls[0]} distance matrices, {time.time() - t:.0f} s", flush=True)
        tu, tw, tk = torch.from_numpy(u), torch.from_numpy(w), torch.from_numpy(np.ascontiguousarray(kp))
        dx, dy = tu[:, None] - tk[None, :, 0], tw[:, None] - tk[None, :, 1]
        return torch.sqrt(dx * dx + dy * dy).min(dim=1)[0].numpy()
    t = time.time()
    retained, kept, trace = CR.select(m["frame_off"], m["row_ids"], m["pt_ids"], m["pt_xyz"], m["xys"], m["cams"], lists, vrf, a.radius,
                                      skip_decided=True, min_dist=min_dist)
    cpu_s = time.time() - t
    print(f"restatement: {cpu_s:.1f} s on {a.threads} threads; {len(retained)} frames retained, {int(kept.sum())} rows kept, "
          f"{trace['tested']} candidates tested, {trace['appended']} appended, {len(trace['lost_all'])} lost every row", flush=True)

    # ---- the device
    from pram_amd import ops
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    store = {"point3D_ids": up(m["row_ids"]), "frame_off": up(m["frame_off"]), "pt_ids": up(m["pt_ids"]), "n_frames": a.frames, "n_rows": n_rows,
             "n_points": len(m["pt_ids"]), "covisibility_frame": a.covisible}
    pt_xyz, xys, cams = up(m["pt_xyz"]), up(m["xys"]), up(m["cams"])
    ws = ops.compress_workspace(store, dev)
    vrf_np = np.array(vrf, dtype=np.int32)
    full = lambda: ops.compress_select(store, m["frame_off"], covis_off, covis_frames, vrf_np, pt_xyz, xys, cams, a.radius, ws)
    # the same launches without work: one row per frame, id -1
    one = np.arange(a.frames + 1, dtype=np.int32)
    idle_store = {**store, "point3D_ids": up(np.full(a.frames, -1, dtype=np.int64)), "frame_off": up(one), "n_rows": a.frames}
    idle_ws, idle_xys = ops.compress_workspace(idle_store, dev), up(np.zeros((a.frames, 2)))
    idle = lambda: ops.compress_select(idle_store, one, covis_off, covis_frames, vrf_np, pt_xyz, idle_xys, cams, a.radius, idle_ws)

    def timed(fn):
        out = fn()
        torch.cuda.synchronize()
        ms, host = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t = time.perf_counter()
            out = fn()
            host.append((time.perf_counter() - t) * 1e3)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return out, ms, host

    (order, cnt, lst), ms, host = timed(full)
    _, idle_ms, idle_host = timed(idle)
    order, cnt = order.cpu().numpy(), cnt.cpu().numpy()
    lst = lst.cpu().numpy()
    place = {f: i for i, f in enumerate(retained)}
    differ = 0
    for f in range(a.frames):
        r0, r1 = int(m["frame_off"][f]), int(m["frame_off"][f + 1])
        same = int(order[f]) == place.get(f, -1)
        if same and f in place:
            same = np.array_equal(m["pt_ids"][lst[r0:r0 + cnt[f]]], m["row_ids"][r0:r1][kept[r0:r1]])
        differ += not same
    print(f"frames differing from the restatement (retained or not, retained order, list): {differ}")
    med = statistics.median
    fmt = lambda v: f"{med(v):.1f} ms ({min(v):.1f} .. {max(v):.1f})"
    print(f"pram_compress_select: device {fmt(ms)}, host enqueue {fmt(host)}; the same {launches} launches without work: device {fmt(idle_ms)}, "
          f"host {fmt(idle_host)}: {100.0 * med(idle_ms) / med(ms):.0f} % of the device time is launch overhead")
    text = f"""# Map compression: selection on the device against the numpy restatement

Written by `python profiles/tools/compress_timing.py --frames {a.frames} --rows {a.rows} --vrfs {a.vrfs} --covisible {a.covisible} --threads {a.threads}`.

| | |
|---|---|
| frames / rows / points | {a.frames} / {n_rows} / {len(m['pt_ids'])} |
| reference frames, covisible_frames, radius | {len(vrf)}, {a.covisible}, {a.radius:g} |
| steps (reference frame, candidate) / launches | {steps} / {launches} |
| candidates tested / appended / lost every row | {trace['tested']} / {trace['appended']} / {len(trace['lost_all'])} |
| frames retained / rows kept | {len(retained)} / {int(kept.sum())} of {n_rows} |
| frames differing from the restatement | **{differ}** |
| `pram_compress_select`, device, median of {a.reps} (min .. max) | {fmt(ms)} |
| host time to enqueue it | {fmt(host)} |
| the same launches without work (one id -1 row per frame), device | {fmt(idle_ms)} |
| share of the device time that is launch overhead | {100.0 * med(idle_ms) / med(ms):.0f} % |
| numpy restatement, distance step in torch on {a.threads} threads, decided rows skipped | {cpu_s:.1f} s |

The restatement is the reference's loop with the reference's torch distance matrix; it is not the reference's program, which also
measures rows that are already discarded.  The launch overhead is measured, not modelled: the idle run enqueues the same begin,
test and commit kernels in the same order on frames that have nothing to test.
"""
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(f"wrote {a.out}")
    return 0 if differ == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
