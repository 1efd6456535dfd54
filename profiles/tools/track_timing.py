"""Timing of the tracker (localization.tracker.Tracker, csrc/track.hip): the four new kernels on their own, and a tracked step
against localize_and_refine on the same batch.

16 streams of 2048 keypoints on refine_projection_timing.py's synthetic map cut to 16 clusters of 5 frames with 2048 rows each
(covisibility_frame 4, seg_k 2).  Stream b looks at cluster b through a planted camera; 1500 of its keypoints are noisy twins of
points of the cluster's first frame, 548 are clutter; the recogniser's logits peak at the cluster's landmark.  The first run call
relocalises every stream; from then on the same frames are tracked (the camera stands still: the cost of a step does not depend
on the motion).

Interleaved repetition by repetition, HIP events around whole calls (their read-backs included), warm:
  track     Tracker.track on the 16 located streams (plan, gather, ONE grouped matcher call of 16 pairs, correspond, pose stage,
            one read-back, commit);
  localize  localize_and_refine on the same batch (32 candidate pairs, then 64 refinement pairs);
and the four kernels, each between its own events, on the state and the matches0 of a tracked step.
    python profiles/tools/track_timing.py [--reps 5] [--dry]"""
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

COVIS, SEG_K, THRESHOLD = 4, 2, 12.0
RP.PER_CLUSTER, RP.COVIS = COVIS + 1, COVIS
B, NQ = RP.B, RP.NQ


def main():
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    reps = int(arg("--reps", 5))
    from pram_amd.localization import candidates as cd
    m, qs, cams, _ = RP.big_scene()
    rng = np.random.default_rng(9)
    for b, q in enumerate(qs):      # the recogniser's output: every keypoint of stream b names landmark b (class b + 1)
        seg = rng.standard_normal((NQ, B + 1)).astype(np.float32)
        seg[:, b + 1] += 8.0
        q["segmentations"] = q["padded"]["segmentations"] = seg
    store = cd.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, covisibility_frame=COVIS)
    print(f"map: {store.n_frames} frames of {store.max_frame_rows} rows, {len(store.pt_ids)} points; {B} streams of {NQ} keypoints, seg_k {SEG_K}, "
          f"covisibility_frame {COVIS}, threshold {THRESHOLD} px", flush=True)
    if "--dry" in sys.argv:
        return
    from pram_amd import ops
    from pram_amd.localization import pose, refine
    from pram_amd.localization.tracker import Tracker
    from pram_amd.nets.gml import GML
    dev = torch.device("cuda:0")
    feats, seg = CR.batch_features(qs, dev)
    dcams = pose.device_cameras(cams, dev)
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    kw = dict(seg_k=SEG_K, min_kpts=32, threshold=THRESHOLD, min_inliers=30, semantic_matching=False)
    trk = Tracker(store, net, B, NQ, covisibility_frame=COVIS, **kw)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    track = lambda: trk.track(feats, dcams)
    localize = lambda: refine.localize_and_refine(feats, seg, store, net, dcams, covisibility_frame=COVIS, **kw)
    with ops.guard_scope("deferred"):
        first = trk.run(feats, seg, dcams)
        print("first call: " + ", ".join(f"{r['source']} {r['num_inliers']}" for r in first), flush=True)
        res = track()
        print("tracked step: " + ", ".join(f"{r['source']} {r['num_inliers']}/{r['tracking']['n_matches']}" if r else "lost" for r in res), flush=True)
        loc = localize()
        # the kernels' inputs, from the state as it stands
        st = trk.state.arrays()
        counts, kp, sc, de = trk._features(feats)
        slot_host = list(range(B))
        slot = torch.arange(B, dtype=torch.int32, device=dev)
        none = torch.full((NQ,), -1, dtype=torch.int64, device=dev)
        matches0 = torch.stack([r["tracking"]["matches0"][:NQ] if r is not None else none for r in res]).contiguous()
        ref = st["ref_frame"].clone()
        winner = torch.empty(B, NQ, device=dev, dtype=torch.int32)
        norm = cd._query_norm(feats)

        def kernels():
            marks = [ev()]
            marks[0].record()
            plan, _ = ops.track_plan(counts, slot, st, NQ)
            marks.append(ev()); marks[-1].record()
            cor = ops.track_correspond(matches0, plan, st, kp, NQ)
            marks.append(ev()); marks[-1].record()
            est_inl = (cor["matched_keypoint_ids"] % 8 != 0).to(torch.uint8)      # a stand-in inlier mask: seven rows of eight
            marks.append(ev()); marks[-1].record()
            kept = ops.track_filter(cor, est_inl)
            marks.append(ev()); marks[-1].record()
            ops.track_commit(st, kp, sc, de, counts, None, slot, slot_host, ref, norm, cor, est_inl, winner)
            marks.append(ev()); marks[-1].record()
            marks[-1].synchronize()
            return [marks[i].elapsed_time(marks[i + 1]) for i in (0, 1, 3, 4)], (cor, kept)

        _, (cor, kept) = kernels()
        torch.cuda.synchronize()
        t = {"kernels": [], "track": [], "localize_and_refine": []}
        for _ in range(reps):
            t["kernels"].append(kernels()[0])
            t["track"].append(timed(track)[0])
            t["localize_and_refine"].append(timed(localize)[0])
    med = statistics.median
    print(f"matches per pair {int(cor['count'].min())} .. {int(cor['count'].max())} of {NQ}; localize_and_refine located "
          f"{sum(r['success'] for r in loc)} of {B}, refined {sum(r['refinement'] is not None for r in loc)}")
    for i, name in enumerate(("pram_track_plan", "pram_track_correspond", "pram_track_filter", "pram_track_commit")):
        v = [r[i] for r in t["kernels"]]
        print(f"  {name}: median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    for k in ("track", "localize_and_refine"):
        print(f"{k}: median {med(t[k]):.3f} ms, min {min(t[k]):.3f}, max {max(t[k]):.3f}, n = {reps}")
    print(f"from the shapes: state {trk.state.nbytes() / 1e6:.1f} MB for {B} slots of {NQ} rows; a commit moves {B * NQ * (128 + 3) * 4 * 2 / 1e6:.1f} MB of "
          f"keypoints, scores and descriptors and writes {B * NQ * (24 + 8 + 4) / 1e6:.2f} MB of point fields; the grouped call has {B} pairs at T = {NQ} "
          f"against {B * SEG_K} + {B * COVIS} for localize_and_refine")


if __name__ == "__main__":
    main()
