"""Times of the two map-building entries (csrc/mapbuild.hip) on a map-like size, beside the numpy restatement of the reference
(tests/mapbuild_ref.py) on the same inputs; the figures of profiles/mapbuild_timing.md.

    python profiles/tools/mapbuild_timing.py [--points 200000] [--frames 2000] [--landmarks 256] [--procs 16] [--out FILE]

The synthetic map: every point belongs to one landmark (a cluster); its track is drawn from a window of frames around the
cluster, length 2 + Exp(6) with 0.5 % of the tracks uniform in 100 .. 400 (drawn from all frames); every observation is one row of
its frame.  The restatement runs first, in --procs forked workers (the reference forks its loop over points the same way), before
the device is touched; then each entry is timed between its own HIP events, warm, with its workspace allocated beforehand.  The
results of the two sides are compared before any figure is printed."""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import mapbuild_ref as MR  # noqa: E402

_G = {}


def make_map(n_points, n_frames, n_landmarks, seed=7):
    rng = np.random.default_rng(seed)
    lens = 2 + np.floor(rng.exponential(6.0, n_points)).astype(np.int64)
    tail = rng.random(n_points) < 0.005
    lens[tail] = rng.integers(100, 401, int(tail.sum()))
    lens = np.minimum(lens, min(400, n_frames))
    label = rng.integers(0, n_landmarks, n_points)
    trk_off = np.zeros(n_points + 1, dtype=np.int32)
    trk_off[1:] = np.cumsum(lens)
    trk_frame = np.zeros(int(trk_off[-1]), dtype=np.int32)
    window = max(64, n_frames // 16)
    for p in range(n_points):
        n = int(lens[p])
        if n > window:
            fr = rng.choice(n_frames, n, replace=False)
        else:
            lo = int(label[p] * (n_frames - window) / max(n_landmarks - 1, 1))
            fr = lo + rng.choice(window, n, replace=False)
        trk_frame[trk_off[p]:trk_off[p + 1]] = fr
    order = np.argsort(trk_frame, kind="stable")      # rows: the observations of a frame in point order
    counts = np.bincount(trk_frame, minlength=n_frames)
    frame_off = np.zeros(n_frames + 1, dtype=np.int32)
    frame_off[1:] = np.cumsum(counts)
    trk_kpt = np.zeros_like(trk_frame)
    trk_kpt[order] = (np.arange(len(order)) - frame_off[trk_frame[order]]).astype(np.int32)
    owner = np.repeat(np.arange(1, n_points + 1, dtype=np.int64), lens)      # point ids 1 .. P
    point3D_ids = owner[order]
    n_rows = len(order)
    centres = rng.standard_normal((n_points, 128)).astype(np.float32)
    d = centres[point3D_ids - 1] + 0.6 * rng.standard_normal((n_rows, 128)).astype(np.float32)
    descriptors = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    landmarks = [np.nonzero(label == l)[0] + 1 for l in range(n_landmarks)]
    xyz = np.concatenate([rng.uniform(-1, 1, (n_points, 2)), np.full((n_points, 1), 5.0)], 1)
    cams = np.zeros((n_frames, 13))
    cams[:, 0], cams[:, 7:11], cams[:, 11], cams[:, 12] = 1.0, MR.INTRINSICS, MR.WIDTH, MR.HEIGHT
    return dict(frame_off=frame_off, descriptors=descriptors, point3D_ids=point3D_ids, trk_off=trk_off, trk_frame=trk_frame, trk_kpt=trk_kpt,
                landmarks=landmarks, xyz=xyz, cams=cams, n_points=n_points, n_frames=n_frames)


def _desc_chunk(bounds):
    m, (a, b) = _G["map"], bounds
    off = m["trk_off"][a:b + 1] - m["trk_off"][a]
    e0, e1 = m["trk_off"][a], m["trk_off"][b]
    return MR.assign_point_descriptors(m["descriptors"], m["frame_off"], off, m["trk_frame"][e0:e1], m["trk_kpt"][e0:e1])[0]


def _vrf_chunk(ids):
    m = _G["map"]
    fo = m["frame_off"]
    frame_point_ids = [m["point3D_ids"][fo[f]:fo[f + 1]] for f in range(m["n_frames"])]
    point_frames = _G["point_frames"]
    xyz = _G["xyz_of"]
    return MR.select_reference_frames([m["landmarks"][l].tolist() for l in ids], frame_point_ids, point_frames, xyz,
                                      np.zeros(m["n_frames"], dtype=np.int32), m["cams"], **_G["params"])[0]


class _Lazy(dict):
    """point id -> value, made when asked for (200k small lists cost more to build than the landmarks ever read)"""

    def __init__(self, fn, n):
        super().__init__()
        self.fn, self.n = fn, n

    def __contains__(self, k):
        return 1 <= k <= self.n

    def __missing__(self, k):
        return self.fn(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--landmarks", type=int, default=256)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    params = dict(min_obs=120, topk_imgs=500, n_vrf=10, min_cover_ratio=0.9, gain_floor=0.01)
    t0 = time.time()
    m = make_map(a.points, a.frames, a.landmarks)
    lens = np.diff(m["trk_off"])
    res = {"points": a.points, "frames": a.frames, "landmarks": a.landmarks, "rows": int(m["frame_off"][-1]), "track_mean": float(lens.mean()),
           "track_max": int(lens.max()), "tracks_over_32": int((lens > 32).sum()), "sum_n2": int((lens.astype(np.int64) ** 2).sum()),
           "procs": a.procs}
    print(f"map made in {time.time() - t0:.1f} s: {res}", flush=True)

    # ---- the restatement, forked before the device is touched
    _G.update(map=m, params=params)
    _G["point_frames"] = _Lazy(lambda p: m["trk_frame"][m["trk_off"][p - 1]:m["trk_off"][p]].tolist(), a.points)
    _G["xyz_of"] = _Lazy(lambda p: m["xyz"][p - 1], a.points)
    cuts = np.searchsorted(np.cumsum(lens.astype(np.int64) ** 2), np.linspace(0, float((lens.astype(np.int64) ** 2).sum()), 4 * a.procs + 1)[1:-1])
    cuts = np.unique(np.concatenate([[0], cuts, [a.points]]))
    with mp.get_context("fork").Pool(a.procs) as pool:
        t = time.time()
        ref_choice = np.concatenate(pool.map(_desc_chunk, list(zip(cuts[:-1].tolist(), cuts[1:].tolist())), chunksize=1))
        res["cpu_desc_s"] = time.time() - t
        print(f"restatement, descriptors: {res['cpu_desc_s']:.2f} s", flush=True)
        t = time.time()
        ref_vrf = sum(pool.map(_vrf_chunk, [[l] for l in range(a.landmarks)], chunksize=1), [])
        res["cpu_vrf_s"] = time.time() - t
        print(f"restatement, reference frames: {res['cpu_vrf_s']:.2f} s", flush=True)

    # ---- the device
    import torch
    from pram_amd import _lib, ops
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    pt_off = m["trk_off"]
    store = {"descriptors": up(m["descriptors"]), "frame_off": up(m["frame_off"]), "point3D_ids": up(m["point3D_ids"]),
             "pt_ids": up(np.arange(1, a.points + 1, dtype=np.int64)), "pt_off": up(pt_off), "pt_frames": up(m["trk_frame"]),
             "n_frames": a.frames, "n_rows": res["rows"], "n_points": a.points, "n_pt_entries": int(pt_off[-1])}
    trk_off, trk_frame, trk_kpt = up(m["trk_off"]), up(m["trk_frame"]), up(m["trk_kpt"])
    lm_off = np.zeros(a.landmarks + 1, dtype=np.int32)
    lm_off[1:] = np.cumsum([len(v) for v in m["landmarks"]])
    lm_off_d, lm_points = up(lm_off), up(np.concatenate(m["landmarks"]).astype(np.int64))
    ignored, cams, pt_xyz = up(np.zeros(a.frames, dtype=np.int32)), up(m["cams"]), up(m["xyz"])
    L = _lib.load()
    import ctypes
    host = (ctypes.c_int * (a.points + 1)).from_buffer_copy(m["trk_off"].tobytes())
    ws_d = torch.empty(max(int(L.pram_mapbuild_desc_workspace_bytes(ctypes.addressof(host), a.points)), 8), device=dev, dtype=torch.uint8)
    ws_v = torch.empty(int(L.pram_mapbuild_vrf_workspace_bytes(a.landmarks, int(lm_off[-1]), a.frames)), device=dev, dtype=torch.uint8)
    res["ws_desc_bytes"], res["ws_vrf_bytes"] = ws_d.numel(), ws_v.numel()
    desc = lambda: ops.mapbuild_assign_descriptors(store, trk_off, m["trk_off"], trk_frame, trk_kpt, workspace=ws_d)
    vrf = lambda: ops.mapbuild_select_frames(store, pt_xyz, lm_off_d, lm_off, lm_points, ignored, cams, workspace=ws_v, **params)

    def timed(fn):
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return out, ms

    (pt_desc, pt_choice), ms_d = timed(desc)
    (lm_vrf, lm_vrf_n), ms_v = timed(vrf)
    choice = pt_choice.cpu().numpy()
    differ = int((choice != ref_choice).sum())
    got_vrf = [lm_vrf[l, :int(n)].tolist() for l, n in enumerate(lm_vrf_n.cpu().tolist())]
    res.update(gpu_desc_ms=ms_d, gpu_vrf_ms=ms_v, desc_choices_differ=differ, vrf_lists_differ=sum(g != w for g, w in zip(got_vrf, ref_vrf)),
               vrf_frames_mean=float(np.mean([len(v) for v in ref_vrf])), gather_bytes=int(lens.sum()) * 512)
    fmt = lambda ms: f"{statistics.median(ms):.3f} ms ({min(ms):.3f} .. {max(ms):.3f})"
    print(f"pram_mapbuild_assign_descriptors: {fmt(ms_d)}; {res['gather_bytes'] / statistics.median(ms_d) / 1e6:.1f} GB/s of gathered rows; "
          f"{differ} of {a.points} choices differ from the restatement")
    print(f"pram_mapbuild_select_frames: {fmt(ms_v)}; {res['vrf_lists_differ']} of {a.landmarks} lists differ; {res['vrf_frames_mean']:.2f} frames per landmark")
    print(f"restatement on {a.procs} processes: descriptors {res['cpu_desc_s']:.2f} s, reference frames {res['cpu_vrf_s']:.2f} s")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
