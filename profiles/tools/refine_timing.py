"""Timing of localization.refine.localize_and_refine against localization.pose.localize_candidates, with the refinement's stages.

16 queries of 2048 keypoints, seg_k = 2, covisibility_frame 20, on a synthetic map in the style of tests/refine_ref.py's
covisible_scene at full size: 240 frames of 600 .. 1376 rows, frame f observing the pool of world points from 100 f on (so every
frame has more than 20 covisible frames), query b seeing 1500 pool points of its own through a planted camera plus 548 clutter
keypoints.  HIP events, warm; three repetitions, the median reported.  The per-stage share comes from events between the stages
of refine_by_matching, which are replayed here call for call (the public function has no hooks).
    python profiles/tools/refine_timing.py [--reps 3]"""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from pram_amd import ops  # noqa: E402
from pram_amd.localization import candidates as cd  # noqa: E402
from pram_amd.localization import pose, refine  # noqa: E402
from pram_amd.nets.gml import GML  # noqa: E402
from tests import cand_ref as CR, helpers as H, pose_ref as PR  # noqa: E402

B, NQ, OWN, SEG_K, COVIS = 16, 2048, 1500, 2, 20
N_FRAMES, STEP, LM = 240, 100, 500
THRESHOLD, MIN_INLIERS, TRIALS = 4.0, 30, 1000
W, Hh = 640, 480


def big_scene(seed=3, noise=0.25):
    rng = np.random.default_rng(seed)
    rows = rng.integers(600, 1377, N_FRAMES)
    rows[0], rows[1] = 1376, 600
    n_pool = int(max(STEP * f + rows[f] for f in range(N_FRAMES)))
    assert n_pool >= B * OWN
    desc = CR._unit(rng.standard_normal((n_pool, 128)))
    xyz = rng.standard_normal((n_pool, 3)) * 10.0
    pix = np.stack([np.floor(rng.uniform(4, W - 4, n_pool)), np.floor(rng.uniform(4, Hh - 4, n_pool))], 1)
    pid = (rng.permutation(10 * n_pool)[:n_pool] + 1000).astype(np.int64)
    label = (np.arange(n_pool) // LM).astype(np.int32)
    cams = []
    for b in range(B):
        cam = PR.PLANTED_CAMERAS[b % len(PR.PLANTED_CAMERAS)]
        c = PR.unify(*PR.camera_row(cam))
        R = PR.random_rotation(rng)
        t = -R @ np.array([150.0 * (b + 1), -220.0, 40.0]) + rng.standard_normal(3)
        own = np.arange(b * OWN, (b + 1) * OWN)
        px = pix[own] + 0.5 + 0.5 * rng.standard_normal((OWN, 2))
        u, v = PR.undistort((px[:, 0] - c[2]) / c[0], (px[:, 1] - c[3]) / c[1], *c[4:])
        z = rng.uniform(3.0, 30.0, OWN)
        xyz[own] = (np.stack([u * z, v * z, z], 1) - t) @ R
        cams.append(cam)
    frames = []
    for f in range(N_FRAMES):
        pts = rng.permutation(np.arange(STEP * f, STEP * f + rows[f]))
        kp = np.clip(pix[pts] + rng.integers(-2, 3, (len(pts), 2)), 0, [W - 1, Hh - 1])
        frames.append({"id": 1000 + f, "keypoints": np.concatenate([kp, rng.uniform(0, 1, (len(pts), 1))], 1).astype(np.float32),
                       "descriptors": CR._unit(desc[pts] + noise / np.sqrt(128.0) * rng.standard_normal((len(pts), 128))), "xyzs": xyz[pts].copy(),
                       "point3D_ids": pid[pts].copy(), "keypoint_segs": label[pts].copy(), "width": W, "height": Hh})
    n_lm = int(label.max()) + 1
    ref_of = lambda l: 1000 + min(l * LM // STEP, N_FRAMES - 1)
    m = {"frames": frames, "seg_ref_frame_ids": {l: [ref_of(l), ref_of((l + 1) % n_lm)] for l in range(n_lm)}, "start_sid": 0}
    qs = []
    for b in range(B):
        own = np.arange(b * OWN, (b + 1) * OWN)
        nc = NQ - OWN
        d = np.concatenate([CR._unit(desc[own] + noise / np.sqrt(128.0) * rng.standard_normal((OWN, 128))), CR._unit(rng.standard_normal((nc, 128)))])
        k = np.concatenate([pix[own], np.stack([np.floor(rng.uniform(4, W - 4, nc)), np.floor(rng.uniform(4, Hh - 4, nc))], 1)])
        cls = np.concatenate([label[own].astype(np.int64) + 1, np.zeros(nc, dtype=np.int64)])
        perm = rng.permutation(NQ)
        seg = rng.standard_normal((NQ, n_lm + 1)).astype(np.float32)
        seg[np.arange(NQ), cls[perm]] += 8.0
        q = {"keypoints": k[perm].astype(np.float32), "scores": rng.uniform(0, 1, NQ).astype(np.float32), "descriptors": d[perm].astype(np.float32),
             "segmentations": seg, "width": W, "height": Hh, "count": NQ}
        q["padded"] = {kk: q[kk] for kk in ("keypoints", "scores", "descriptors", "segmentations")}
        qs.append(q)
    return m, qs, cams


def main():
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    reps = int(arg("--reps", 3))
    dev = torch.device("cuda:0")
    m, qs, cams = big_scene()
    store = cd.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, device=dev, covisibility_frame=COVIS)
    lens = np.diff(store.covis_off)[store.is_vrf.astype(bool)]
    print(f"map: {store.n_frames} frames, {store.n_rows} rows ({np.diff(store.frame_off).min()} .. {np.diff(store.frame_off).max()} per frame), "
          f"{len(store.pt_ids)} points, {int(store.is_vrf.sum())} vrf frames with {lens.min()} .. {lens.max()} covisible frames")
    feats, seg = CR.batch_features(qs, dev)
    cams = pose.device_cameras(cams, dev)
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    kw = dict(seg_k=SEG_K, min_kpts=32, threshold=THRESHOLD, min_inliers=MIN_INLIERS, trials=TRIALS, semantic_matching=False)
    full = dict(kw, overlap_ratio=0.5, min_inlier_ratio=0.01, refine_iters=20, seed=0)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def staged():
        """refine_by_matching's stages with an event after each -> (names, events)"""
        _, st = pose._localize(feats, seg, store, net, cams, **full)
        marks = [("localize", ev())]
        marks[-1][1].record()
        tables = store.tables(dev)
        plan, ref_frame, used, init_on = ops.refine_plan(st["chosen"], st["plan"], feats["counts"], tables, COVIS)
        marks.append(("plan", ev())); marks[-1][1].record()
        data = cd.gather_candidates(feats, {"plan": plan, "vote": {"tokens": st["tokens"]}}, store)
        t0 = data.pop("t0"); data.pop("plan_host")
        marks.append(("plan read-back + gather", ev())); marks[-1][1].record()
        mm = net.produce_matches(data)
        marks.append(("matcher", ev())); marks[-1][1].record()
        cor = ops.cand_correspond(mm["matches0"][:, :t0], plan, st["tokens"], tables, feats["keypoints"].contiguous(), t0)
        marks.append(("correspond", ev())); marks[-1][1].record()
        merged = ops.refine_merge(cor, st["cor"], st["chosen"], init_on, COVIS)
        marks.append(("merge", ev())); marks[-1][1].record()
        est = pose.estimate_poses(merged["matched_keypoints"], merged["matched_xyzs"], merged["count"], cams, seg_k=1, threshold=THRESHOLD, trials=TRIALS)
        marks.append(("pose", ev())); marks[-1][1].record()
        bf, _, nb = ops.refine_frame_vote(merged["matched_point3D_ids"], merged["count"], est["inliers"], est["success"], tables, COVIS)
        marks.append(("frame vote", ev())); marks[-1][1].record()
        torch.cat([est["qvec"], est["tvec"], bf.double()], 1).cpu()
        marks.append(("read-back", ev())); marks[-1][1].record()
        marks[-1][1].synchronize()
        return marks, data["descriptors0"].shape

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    loc = lambda: pose.localize_candidates(feats, seg, store, net, cams, **kw)
    both = lambda: refine.localize_and_refine(feats, seg, store, net, cams, **kw)
    with ops.guard_scope("deferred"):
        res = both()
        loc()
        staged()
        torch.cuda.synchronize()
        t = {"localize_candidates": [], "localize_and_refine": []}
        stages = []
        for _ in range(reps):
            t["localize_candidates"].append(timed(loc)[0])
            t["localize_and_refine"].append(timed(both)[0])
            marks, shape = staged()
            stages.append({name: marks[i][1].elapsed_time(e) for i, (name, e) in enumerate(marks[1:])})
    med = statistics.median
    ref = [r["refinement"] for r in res if r["refinement"] is not None]
    print(f"grouped call of the refinement: {shape[0]} pairs at T = {shape[1]}; refined queries {len(ref)} of {B}, tracked "
          f"{sum(r['tracking_status'] is True for r in res)}, refinements with a pose {sum(x['success'] for x in ref)}")
    print("inliers localisation -> refinement: " + ", ".join(f"{r['num_inliers']} -> {r['refinement']['num_inliers']}" for r in res if r["refinement"]))
    for k, v in t.items():
        print(f"{k}: median {med(v):.2f} ms, min {min(v):.2f}, max {max(v):.2f}, n = {len(v)}")
    total = sum(med([s[name] for s in stages]) for name in stages[0])
    for name in stages[0]:
        v = med([s[name] for s in stages])
        print(f"  refinement stage {name}: median {v:.3f} ms ({100 * v / total:.1f} % of the refinement's {total:.2f} ms)")


if __name__ == "__main__":
    main()
