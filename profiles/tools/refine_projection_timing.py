"""Timing of the refinement by projection (localization.refine.refine_by_projection, csrc/projref.hip) against the dense path it
replaces and against refine_by_matching on the same batch.

16 queries of 2048 keypoints, covisibility_frame 20, on a synthetic map of 16 clusters of 21 frames with 2048 rows each: 1900 rows
of a frame are its own points, 148 are the cluster's shared points, so every frame of a cluster is covisible with the 20 others
and the 21 frames hold 40 048 unique points.  Query b looks at cluster b through a planted camera that sees all of the cluster's
points; 1500 of its keypoints are noisy twins of points of the cluster's first frame, 548 are clutter.  The localisation's state
is written by hand from the planted pose (no network runs in the projection form).

Three things, interleaved repetition by repetition, HIP events, warm:
  fused    the four new kernels (mark, project, match, correspond), each between its own events;
  dense    per query: gather of the candidates' descriptors, bgemm_nt [2048, n_cand], pram_proj_dist_top2_f64uv, on the candidates
           the fused path produced;
  matching refine_by_matching (GML, split-fp16) on the same batch and state.
and refine_by_projection as a whole (its pose stage, frame vote and read-back included).  The tool counts the keypoints that the
fused and the dense path decide differently (they sum the 128 products in different orders) and reports the count.
    python profiles/tools/refine_projection_timing.py [--reps 5] [--threshold 12] [--dry]"""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import cand_ref as CR, helpers as H, pose_ref as PR  # noqa: E402

B, NQ, OWN_Q, COVIS, SEG_K = 16, 2048, 1500, 20, 2
ROWS, SHARED, PER_CLUSTER = 2048, 148, 21
W, Hh = 640, 480


def big_scene(seed=5, noise=0.25):
    rng = np.random.default_rng(seed)
    own_rows = ROWS - SHARED
    n_cluster = PER_CLUSTER * own_rows + SHARED
    n_pool = B * n_cluster
    desc = CR._unit(rng.standard_normal((n_pool, 128)))
    pid = (rng.permutation(10 * n_pool)[:n_pool] + 1000).astype(np.int64)
    pix = np.stack([np.floor(rng.uniform(4, W - 4, n_pool)), np.floor(rng.uniform(4, Hh - 4, n_pool))], 1)
    xyz = np.zeros((n_pool, 3))
    cams, poses, frames, queries, seg_ref = [], [], [], [], {}
    for b in range(B):
        cam = PR.PLANTED_CAMERAS[b % len(PR.PLANTED_CAMERAS)]
        c = PR.unify(*PR.camera_row(cam))
        R = PR.random_rotation(rng)
        t = -R @ np.array([150.0 * (b + 1), -220.0, 40.0]) + rng.standard_normal(3)
        pts = np.arange(b * n_cluster, (b + 1) * n_cluster)
        px = pix[pts] + 0.5 + 0.5 * rng.standard_normal((n_cluster, 2))
        u, v = PR.undistort((px[:, 0] - c[2]) / c[0], (px[:, 1] - c[3]) / c[1], *c[4:])
        z = rng.uniform(3.0, 30.0, n_cluster)
        xyz[pts] = (np.stack([u * z, v * z, z], 1) - t) @ R
        cams.append(cam)
        poses.append((PR.rot_to_qvec(R), t))
        shared = pts[-SHARED:]
        for f in range(PER_CLUSTER):
            rows = rng.permutation(np.concatenate([pts[f * own_rows:(f + 1) * own_rows], shared]))
            kp = np.clip(pix[rows] + rng.integers(-2, 3, (ROWS, 2)), 0, [W - 1, Hh - 1])
            frames.append({"id": 1000 + b * PER_CLUSTER + f, "keypoints": np.concatenate([kp, rng.uniform(0, 1, (ROWS, 1))], 1).astype(np.float32),
                           "descriptors": CR._unit(desc[rows] + noise / np.sqrt(128.0) * rng.standard_normal((ROWS, 128))), "xyzs": xyz[rows].copy(),
                           "point3D_ids": pid[rows].copy(), "keypoint_segs": np.full(ROWS, b, np.int32), "width": W, "height": Hh})
        seg_ref[b] = [1000 + b * PER_CLUSTER + f for f in range(PER_CLUSTER)]
        own = pts[:OWN_Q]
        nc = NQ - OWN_Q
        d = np.concatenate([CR._unit(desc[own] + noise / np.sqrt(128.0) * rng.standard_normal((OWN_Q, 128))), CR._unit(rng.standard_normal((nc, 128)))])
        k = np.concatenate([pix[own], np.stack([np.floor(rng.uniform(4, W - 4, nc)), np.floor(rng.uniform(4, Hh - 4, nc))], 1)])
        perm = rng.permutation(NQ)
        q = {"keypoints": k[perm].astype(np.float32), "scores": rng.uniform(0, 1, NQ).astype(np.float32), "descriptors": d[perm].astype(np.float32),
             "segmentations": np.zeros((NQ, 2), np.float32), "width": W, "height": Hh, "count": NQ}
        q["padded"] = {kk: q[kk] for kk in ("keypoints", "scores", "descriptors", "segmentations")}
        queries.append(q)
    return {"frames": frames, "seg_ref_frame_ids": seg_ref, "start_sid": 0}, queries, cams, poses


def main():
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    reps, threshold = int(arg("--reps", 5)), float(arg("--threshold", 12.0))
    from pram_amd.localization import candidates as cd
    m, qs, cams, poses = big_scene()
    store = cd.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, covisibility_frame=COVIS)
    lens = np.diff(store.covis_off)[store.is_vrf.astype(bool)]
    cap = min(len(store.pt_ids), (COVIS + 1) * store.max_frame_rows)
    print(f"map: {store.n_frames} frames of {store.max_frame_rows} rows, {len(store.pt_ids)} points, covisible lists of {lens.min()} .. {lens.max()} frames; "
          f"candidates per query at most {cap}; threshold {threshold} px", flush=True)
    if "--dry" in sys.argv:
        return
    from pram_amd import ops
    from pram_amd.localization import pose, refine
    from pram_amd.nets.gml import GML
    dev = torch.device("cuda:0")
    tables = store.point_tables(dev)
    feats, _ = CR.batch_features(qs, dev)
    dcams = pose.device_cameras(cams, dev)
    sizes = torch.from_numpy(refine.image_size_table(cams)).to(dev)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    # the localisation's state, by hand: candidate 0 kept, tracked, the cluster's first frame, the planted pose
    chosen = np.tile(np.array([[0, 1, 0]], np.int32), (B, 1))
    plan = np.zeros((ops.CAND_PLAN_COLS, B * SEG_K), np.int32)
    plan[ops.CAND_PLAN_FIELDS.index("frame"), ::SEG_K] = np.arange(B) * PER_CLUSTER
    qv, tv = np.zeros((B * SEG_K, 4)), np.zeros((B * SEG_K, 3))
    for b, (q, t) in enumerate(poses):
        qv[b * SEG_K], tv[b * SEG_K] = q, t
    est = {"qvec": torch.from_numpy(qv).to(dev), "tvec": torch.from_numpy(tv).to(dev)}
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    P = B * SEG_K
    cor = {"matched_keypoint_ids": z((P, 1), torch.int64), "matched_keypoints": z((P, 1, 2), torch.float32), "matched_ref_keypoints": z((P, 1, 2), torch.float32),
           "matched_point3D_ids": z((P, 1), torch.int64), "matched_xyzs": z((P, 1, 3), torch.float64), "matched_sids": z((P, 1), torch.int32), "count": z((P,), torch.int32)}
    state = {"chosen": i32(chosen), "plan": i32(plan), "tokens": z((B, SEG_K, NQ), torch.int32), "cor": cor, "est": est, "seg_k": SEG_K}
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    kpts, descs, counts = feats["keypoints"].contiguous(), feats["descriptors"].contiguous(), feats["counts"].contiguous()
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def fused():
        marks = [ev()]
        marks[0].record()
        bitmap, _ = ops.projref_mark(state["chosen"], state["plan"], tables, COVIS)
        marks.append(ev()); marks[-1].record()
        cand_pt, cand_uv, n_union, n_cand = ops.projref_project(bitmap, state["chosen"], est["qvec"], est["tvec"], dcams[0], dcams[1], sizes, tables, cap)
        marks.append(ev()); marks[-1].record()
        best, d0, d1, accept = ops.projref_match(kpts, descs, counts, cand_pt, cand_uv, n_cand, tables, threshold)
        marks.append(ev()); marks[-1].record()
        out = ops.projref_correspond(accept, best, counts, kpts, cand_pt, n_cand, tables)
        marks.append(ev()); marks[-1].record()
        marks[-1].synchronize()
        return [marks[i].elapsed_time(marks[i + 1]) for i in range(4)], (cand_pt, cand_uv, n_union, n_cand, best, accept, out)

    def dense(cand_pt, cand_uv, n_host):
        a, b = ev(), ev()
        a.record()
        res = []
        for q in range(B):
            n = n_host[q]
            rd = tables["pt_desc"][cand_pt[q, :n].long()].contiguous()
            sim = ops.bgemm_nt(descs[q][None], rd[None], ldc=(n + 3) // 4 * 4)[0]
            d0, d1, i0 = ops.proj_dist_top2_f64uv(sim, kpts[q], cand_uv[q], 2.0 * threshold, n)
            res.append(((d0 / d1 <= 0.995) & (d0 < 100), i0))
        b.record()
        b.synchronize()
        return a.elapsed_time(b), res

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    by_proj = lambda: refine.refine_by_projection(feats, state, store, dcams, threshold=threshold, covisibility_frame=COVIS, image_sizes=sizes)
    by_match = lambda: refine.refine_by_matching(feats, state, store, net, dcams, threshold=threshold, covisibility_frame=COVIS)
    with ops.guard_scope("deferred"):
        _, (cand_pt, cand_uv, n_union, n_cand, best, accept, out) = fused()
        n_host = [int(v) for v in n_cand.cpu()]
        _, dres = dense(cand_pt, cand_uv, n_host)
        differ = 0      # faster and different is not faster: keypoints the two paths decide differently (they sum in different orders)
        for q in range(B):
            ok = accept[q].bool()
            differ += int((ok != dres[q][0]).sum()) + int((best[q].long() != dres[q][1])[ok & dres[q][0]].sum())
        rp, rm = by_proj(), by_match()
        torch.cuda.synchronize()
        t = {"fused": [], "dense": [], "refine_by_projection": [], "refine_by_matching": []}
        for _ in range(reps):
            t["fused"].append(fused()[0])
            t["dense"].append(dense(cand_pt, cand_uv, n_host)[0])
            t["refine_by_projection"].append(timed(by_proj)[0])
            t["refine_by_matching"].append(timed(by_match)[0])
    med = statistics.median
    print(f"union per query {int(n_union.min())} .. {int(n_union.max())}, candidates {min(n_host)} .. {max(n_host)}, accepted keypoints "
          f"{int(out['count'].min())} .. {int(out['count'].max())} of {NQ}; keypoints the fused and the dense path decide differently: {differ} of {B * NQ}")
    print("inliers / matches, projection: " + ", ".join(f"{x['num_inliers']}/{x['matched_keypoints'].shape[0]}" for x in rp if x))
    print("inliers / matches, matching:   " + ", ".join(f"{x['num_inliers']}/{x['matched_keypoints'].shape[0]}" for x in rm if x))
    for i, name in enumerate(("mark", "project", "match", "correspond")):
        v = [r[i] for r in t["fused"]]
        print(f"  kernel stage {name}: median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}")
    tot = [sum(r) for r in t["fused"]]
    print(f"fused, four kernels: median {med(tot):.3f} ms, min {min(tot):.3f}, max {max(tot):.3f}, n = {reps}")
    for k in ("dense", "refine_by_projection", "refine_by_matching"):
        print(f"{k}: median {med(t[k]):.3f} ms, min {min(t[k]):.3f}, max {max(t[k]):.3f}, n = {reps}")
    c = float(np.mean(n_host))
    print(f"from the shapes: dense similarity matrices {B * NQ * c * 4 / 1e6:.0f} MB and {2 * B * NQ * c * 128 / 1e9:.1f} GFLOP per batch; "
          f"fused range tests {B * NQ * c / 1e9:.2f}e9, outputs {B * NQ * 13 / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
