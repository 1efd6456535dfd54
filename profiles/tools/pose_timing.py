"""Timing of localization.pose.localize_candidates and of match_candidates before / after its refactoring.

The 80-pair case of candidates_timing.py (B = 16 queries of 512 keypoints, seg_k = 5, the seeded synthetic map of
tests/cand_ref.py), with one planted camera per query (tests/pose_ref.plant_cameras) so that the pose stage has poses to find.
HIP events, warm, the paths alternating in one process; prints medians and each path's own spread.
    python profiles/tools/pose_timing.py [--reps 24] [--parent FILE] [--once] [--cpu-restatement]
--parent FILE: the parent commit's pram_amd/localization/candidates.py (git show PARENT:pram_amd/localization/candidates.py > FILE),
               loaded beside this commit's and timed interleaved with it;
--once: two public calls and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ... --once);
--cpu-restatement: also time tests/pose_ref.estimate_pose on the same 80 pairs (an unoptimised numpy port, NOT the reference)."""
import importlib.util
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from pram_amd import ops  # noqa: E402
from pram_amd.localization import candidates as cd  # noqa: E402
from pram_amd.localization import pose  # noqa: E402
from pram_amd.nets.gml import GML  # noqa: E402
from tests import cand_ref as CR, helpers as H, pose_ref as PR  # noqa: E402

B, SEG_K, MIN_KPTS, NQ = 16, 5, 32, 512
THRESHOLD, MIN_INLIERS, TRIALS = 4.0, 30, 1000


def main():
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    reps = int(arg("--reps", 24))
    dev = torch.device("cuda:0")
    m = CR.make_map(41)
    nf = len(m["frames"])
    qs = []
    for b in range(B):
        f = 2 + b % (nf - 4)
        qs.append(CR.make_query(50 + b, m, [(2 * f, 200), (2 * f + 1, 150), (2 * f + 2, 60), (2 * ((f + 3) % nf), 40), (2 * ((f + 5) % nf) + 1, 20),
                                           (None, 42)], NQ, CR.N_CLASS))
    planted = PR.plant_cameras(m, qs, seed=1)
    cams = [p["cam"] for p in planted]
    store = cd.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, device=dev)
    feats, seg = CR.batch_features(qs, dev)
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    kw = dict(seg_k=SEG_K, min_kpts=MIN_KPTS)
    paths = {"match_candidates (this commit)": lambda: cd.match_candidates(feats, seg, store, net, **kw)}
    if arg("--parent"):
        spec = importlib.util.spec_from_file_location("parent_candidates", arg("--parent"))
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        pstore = parent.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, device=dev)
        paths["match_candidates (parent commit)"] = lambda: parent.match_candidates(feats, seg, pstore, net, **kw)
    loc = lambda: pose.localize_candidates(feats, seg, store, net, cams, threshold=THRESHOLD, min_inliers=MIN_INLIERS, trials=TRIALS, **kw)
    paths["localize_candidates"] = loc

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    with ops.guard_scope("deferred"):
        res = loc()
        torch.cuda.synchronize()
        if "--once" in sys.argv:
            loc()
            torch.cuda.synchronize()
            return
        for _ in range(3):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in paths}
        for _ in range(reps):
            for k, fn in paths.items():
                t[k].append(timed(fn))
    med = statistics.median
    cands = [c for r in res for c in r["candidates"]]
    print(f"pairs {len(cands)}, matches {sum(c['n_matches_host'] for c in cands)} (per pair {min(c['n_matches_host'] for c in cands)}.."
          f"{max(c['n_matches_host'] for c in cands)}), pairs with a pose {sum(c['success'] for c in cands)}, "
          f"tracked queries {sum(r['tracking_status'] is True for r in res)} of {B}, trials {TRIALS}")
    for k, v in t.items():
        print(f"{k}: median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}, spread (max - min) / median {100 * (max(v) - min(v)) / med(v):.2f} %, n = {len(v)}")
    if arg("--parent"):
        a, b = med(t["match_candidates (this commit)"]), med(t["match_candidates (parent commit)"])
        print(f"match_candidates, ratio of medians this / parent: {a / b:.4f}")
    print(f"pose stage (localize_candidates - match_candidates, medians): {med(t['localize_candidates']) - med(t['match_candidates (this commit)']):.3f} ms")
    if "--cpu-restatement" in sys.argv:
        trimmed = [(c["matched_keypoints"][:c["n_matches_host"]].cpu().numpy(), c["matched_xyzs"][:c["n_matches_host"]].cpu().numpy()) for c in cands]
        t0 = time.perf_counter()
        for p, (k, x) in enumerate(trimmed):
            PR.estimate_pose(k, x, cams[p // SEG_K], threshold=THRESHOLD, trials=TRIALS, p=p)
        print(f"numpy restatement (tests/pose_ref.py, an unoptimised port, not the reference), the same {len(trimmed)} pairs on the host: "
              f"{1e3 * (time.perf_counter() - t0):.0f} ms")


if __name__ == "__main__":
    main()
