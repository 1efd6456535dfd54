"""Timing of the query pre-filter (csrc/prefilter.hip) and of a Localizer step with and without it.

track_timing.py's scene: 16 streams of 2048 keypoints on refine_projection_timing.py's synthetic map cut to 16 clusters of 5
frames (covisibility_frame 4, seg_k 2).  1500 keypoints of stream b are noisy twins of points of cluster b, 548 are clutter.  The
recogniser's logits have 113 classes: a twin peaks at the cluster's landmark, a clutter row at the background, so at
pre_filtering_th = 0.95 every frame fires and keeps its 1500 twins and a few clutter rows (about 74 %).

Interleaved repetition by repetition, HIP events around whole calls (their read-backs included), warm:
  prefilter   pram_query_prefilter on its own (ops.query_prefilter on the recogniser epilogue's outputs);
  step 0.95   Localizer.run_features, tracking, the filter at 0.95 (the tracked step sees about 1520 rows per stream);
  step 0      the same with pre_filtering_th = 0 (2048 rows per stream).
Both localizers are first brought to the tracking state by one call each.
    python profiles/tools/localizer_timing.py [--reps 5] [--dry]"""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import refine_projection_timing as RP  # noqa: E402
from tests import cand_ref as CR, helpers as H  # noqa: E402

COVIS, SEG_K, THRESHOLD, N_CLASS, TH = 4, 2, 12.0, 113, 0.95
RP.PER_CLUSTER, RP.COVIS = COVIS + 1, COVIS
B, NQ = RP.B, RP.NQ


def main():
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    reps = int(arg("--reps", 5))
    from pram_amd.localization import candidates as cd
    m, qs, cams, _ = RP.big_scene()
    rng = np.random.default_rng(9)
    n_twins = []
    for b, q in enumerate(qs):      # a twin (a descriptor close to one of the cluster's rows) names landmark b, a clutter row the background
        rows = np.concatenate([f["descriptors"] for f in m["frames"][b * RP.PER_CLUSTER:(b + 1) * RP.PER_CLUSTER]])
        twin = (q["descriptors"] @ rows.T).max(1) > 0.6
        seg = rng.standard_normal((NQ, N_CLASS)).astype(np.float32)
        seg[np.arange(NQ), np.where(twin, b + 1, 0)] += 10.0
        q["segmentations"] = q["padded"]["segmentations"] = seg
        n_twins.append(int(twin.sum()))
    store = cd.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, covisibility_frame=COVIS)
    print(f"map: {store.n_frames} frames of {store.max_frame_rows} rows; {B} streams of {NQ} keypoints ({min(n_twins)} .. {max(n_twins)} twins), {N_CLASS} classes, "
          f"seg_k {SEG_K}, covisibility_frame {COVIS}, threshold {THRESHOLD} px", flush=True)
    if "--dry" in sys.argv:
        return
    from pram_amd import ops
    from pram_amd.localization import pose
    from pram_amd.localization.localizer import Localizer
    from pram_amd.nets.gml import GML
    from pram_amd.pipeline import QueryPipeline
    dev = torch.device("cuda:0")
    feats, seg = CR.batch_features(qs, dev)
    dcams = pose.device_cameras(cams, dev)
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    pipe = QueryPipeline(None, None, net, guard="deferred")
    kw = dict(seg_k=SEG_K, min_kpts=32, threshold=THRESHOLD, min_inliers=30, semantic_matching=False, covisibility_frame=COVIS)
    on = Localizer(pipe, store, pre_filtering_th=TH, tracking=True, n_streams=B, n_max=NQ, **kw)
    off = Localizer(pipe, store, pre_filtering_th=0.0, tracking=True, n_streams=B, n_max=NQ, **kw)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    ids, mask, cnt, _ = ops.seg_epilogue(seg, feats["counts"], TH)
    kernel = lambda: ops.query_prefilter(feats["keypoints"], feats["scores"], feats["descriptors"], seg, ids, mask, cnt, feats["counts"], True)
    step_on = lambda: on.run_features(feats, seg, dcams)
    step_off = lambda: off.run_features(feats, seg, dcams)
    for name, fn in (("0.95", step_on), ("0", step_off)):
        first = fn()
        print(f"first call, th {name}: " + ", ".join(f"{r['source']} {r['num_inliers']}" for r in first), flush=True)
        res = fn()
        print(f"tracked step, th {name}: " + ", ".join(f"{r['source']} {r['num_inliers']} {r['n_keypoints'][1]}/{r['n_keypoints'][0]}" for r in res), flush=True)
    out = kernel()
    torch.cuda.synchronize()
    t = {"prefilter": [], "step 0.95": [], "step 0": []}
    for _ in range(reps):
        t["prefilter"].append(timed(kernel)[0])
        t["step 0.95"].append(timed(step_on)[0])
        t["step 0"].append(timed(step_off)[0])
    med = statistics.median
    kept = int(out["counts"].sum())
    row = (2 + 1 + 128 + N_CLASS + 1) * 4
    moved = B * NQ * (4 + 4) + kept * row + B * NQ * row + B * NQ * 4      # mask in, kept out and in; kept rows in; every output row written
    for k in t:
        print(f"{k}: median {med(t[k]):.3f} ms, min {min(t[k]):.3f}, max {max(t[k]):.3f}, n = {reps}")
    print(f"pram_query_prefilter keeps {kept} of {B * NQ} rows of {row} bytes and moves {moved / 1e6:.1f} MB: {moved / 1e6 / med(t['prefilter']):.1f} GB/s at the median")
    print(f"a tracked step with the filter takes {med(t['step 0.95']) / med(t['step 0']):.2f} of the step without it")


if __name__ == "__main__":
    main()
