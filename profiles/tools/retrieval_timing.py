"""Timing of localization.retrieval.localize_by_retrieval, stage by stage, at one production-like shape.

16 queries of 2048 keypoints, 20 retrieved frames each, on refine_timing.py's synthetic map (240 frames of 600 .. 1376 rows, all
of them carrying a point, about 1000 on average; frame f observes the pool of world points from 100 f on; query b sees 1500 pool
points of its own through a planted camera plus 548 clutter keypoints).  A query's retrieval list is the 20 frames starting five
before the first that sees its window, so the first frames overlap it little and the accepted frame is not slot 0.  GML on the
tests' synthetic weights.  HIP events around work that ends in a synchronise, warm; the median of --reps repetitions.  The
per-stage share comes from events between the stages of the 'hloc' and 'iterative' forms, replayed here call for call (the public
function has no hooks).  The cost of solving all slots against the reference's early stop: the public 'iterative' call on the full
lists against the same call on lists cut after the slot it accepted — the least a batched early stop could do.
    python profiles/tools/retrieval_timing.py [--reps 5]"""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from pram_amd import ops  # noqa: E402
from pram_amd.localization import candidates as cd  # noqa: E402
from pram_amd.localization import pose, retrieval as rt  # noqa: E402
from pram_amd.nets.gml import GML  # noqa: E402
from tests import cand_ref as CR, helpers as H  # noqa: E402
import refine_timing as RTM  # noqa: E402

N_DB, OBS_TH, INLIER_TH, COVIS = 20, 3, 50, 20
THRESHOLD, TRIALS = 4.0, 1000


def main():
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    reps = int(arg("--reps", 5))
    dev = torch.device("cuda:0")
    m, qs, cams = RTM.big_scene()
    B = len(qs)
    store = rt.DatabaseStore(m["frames"], device=dev)
    lists = [[1000 + f for f in range(max(0, 15 * b - 5), max(0, 15 * b - 5) + N_DB)] for b in range(B)]
    nv = np.diff(store.valid_off)
    print(f"map: {store.n_frames} frames, {store.n_rows} rows, valid rows per frame {nv.min()} .. {nv.max()} (mean {nv.mean():.0f}), {len(store.pt_ids)} points; "
          f"{B} queries of {qs[0]['count']} keypoints, {N_DB} retrieved frames each")
    feats, _ = CR.batch_features(qs, dev)
    cams = pose.device_cameras(cams, dev)
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    kw = dict(threshold=THRESHOLD, trials=TRIALS, obs_th=OBS_TH, inlier_th=INLIER_TH, covisibility_frame=COVIS)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    tables = store.tables(dev)
    table = torch.tensor([store.indices(l) for l in lists], dtype=torch.int32, device=dev)
    counts = feats["counts"].contiguous()

    def staged(method):
        marks = [("start", ev())]
        marks[-1][1].record()

        def mark(name):
            marks.append((name, ev()))
            marks[-1][1].record()
        plan = ops.retr_plan(table, counts, tables)
        mark("plan")
        dummy = torch.zeros(1, device=dev, dtype=torch.int32)
        view = rt._ValidRowsView(store)
        data = cd.gather_candidates(feats, {"plan": plan, "vote": {"tokens": dummy}}, view)
        t0 = data.pop("t0"); data.pop("plan_host")
        mark("plan read-back + gather")
        mm = net.produce_matches(data)
        mark("matcher")
        cor = ops.cand_correspond(mm["matches0"][:, :t0], plan, dummy, view.tables(dev), feats["keypoints"].contiguous(), t0)
        mark("correspond")
        flt = ops.retr_filter(cor, tables, OBS_TH)
        mark("filter")
        if method == "hloc":
            stack = rt._stack(flt, N_DB)
            mark("stack")
            est = pose.estimate_poses(stack["matched_keypoints"], stack["matched_xyzs"], stack["count"], cams, seg_k=1, threshold=THRESHOLD, trials=TRIALS)
            mark("pose (one per query)")
            order = rt._inlier_order(est["inliers"])
            rt._host({"qvec": est["qvec"], "tvec": est["tvec"], "success": est["success"], "num_inliers": est["num_inliers"], "count": stack["count"]})
        else:
            est = pose.estimate_poses(flt["matched_keypoints"], flt["matched_xyzs"], flt["count"], cams, seg_k=N_DB, threshold=THRESHOLD, trials=TRIALS)
            mark("pose (one per pair)")
            chosen = ops.retr_select(est["success"], est["num_inliers"], flt["count"], N_DB, INLIER_TH, 10)
            mark("select")
            order = rt._inlier_order(est["inliers"])
            rt._host({"qvec": est["qvec"], "tvec": est["tvec"], "success": est["success"], "num_inliers": est["num_inliers"], "count": flt["count"], "chosen": chosen})
        mark("inlier order + read-back")
        marks[-1][1].synchronize()
        del order
        return marks, data["descriptors0"].shape

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    call = lambda method, ls=lists, **extra: rt.localize_by_retrieval(feats, ls, store, net, cams, method=method, **kw, **extra)
    med = statistics.median
    with ops.guard_scope("deferred"):
        res_h, res_i, res_o = call("hloc"), call("iterative"), call("iterative", do_covisibility_opt=True)
        cut = [l[:max(r["order"], 1)] if r["success"] and r["status"] == 1 else l for l, r in zip(lists, res_i)]
        call("iterative", cut)
        staged("hloc"); staged("iterative")
        torch.cuda.synchronize()
        t = {"hloc": [], "iterative": [], "iterative, lists cut at the accepted slot": [], "iterative + do_covisibility_opt": []}
        stages = {"hloc": [], "iterative": []}
        for _ in range(reps):
            t["hloc"].append(timed(lambda: call("hloc"))[0])
            t["iterative"].append(timed(lambda: call("iterative"))[0])
            t["iterative, lists cut at the accepted slot"].append(timed(lambda: call("iterative", cut))[0])
            t["iterative + do_covisibility_opt"].append(timed(lambda: call("iterative", do_covisibility_opt=True))[0])
            for method in stages:
                marks, shape = staged(method)
                stages[method].append({name: marks[i][1].elapsed_time(e) for i, (name, e) in enumerate(marks[1:])})
    print(f"grouped call: {shape[0]} pairs at T = {shape[1]}")
    print("hloc: inliers / stacked rows " + ", ".join(f"{r['num_inliers']}/{r['matched_keypoints'].shape[0]}" for r in res_h))
    print("iterative: (status, accepted slot, inliers) " + ", ".join(f"({r['status']}, {r['order'] - 1}, {r['num_inliers']})" for r in res_i))
    print("iterative + covis: inliers " + ", ".join(str(r["num_inliers"]) for r in res_o))
    print(f"pairs matched and solved: all slots {B * N_DB}, up to the accepted slot {sum(len(c) for c in cut)}")
    # the sampler's pair index is query * n_db + slot and n_db differs, so the inlier counts may differ by a few; the choice must not
    same = all(a["status"] == b["status"] and a["order"] == b["order"] for a, b in zip(res_i, call("iterative", cut)))
    print(f"the cut lists choose the same slot: {same}")
    for k, v in t.items():
        print(f"{k}: median {med(v):.2f} ms, min {min(v):.2f}, max {max(v):.2f}, n = {len(v)}")
    for method, runs in stages.items():
        total = sum(med([s[name] for s in runs]) for name in runs[0])
        for name in runs[0]:
            v = med([s[name] for s in runs])
            print(f"  {method} stage {name}: median {v:.3f} ms ({100 * v / total:.1f} % of {total:.2f} ms)")


if __name__ == "__main__":
    main()
