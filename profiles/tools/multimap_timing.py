"""Timing of localize_candidates against a one-map ReferenceStore, the same map behind a MultiMapStore, and a MultiMapStore of seven
maps; and of the two plan entries (pram_cand_plan, pram_cand_plan_maps) alone.

B = 16 queries of 2048 keypoints, seg_k = 5 (80 pairs), every query twinned from five landmarks of map A (the seeded synthetic map
of tests/cand_ref.py); the recogniser's output has 197 classes (7 maps x 28 landmarks + background) for all three stores, so the
sort and the vote do the same work.  HIP events, warm, the stores alternating inside each repetition, five repetitions, medians.
    python profiles/tools/multimap_timing.py [--reps 5] [--single]      (--single: ReferenceStore(A) only; runs on a tree without
                                                                          MultiMapStore, for the comparison with the parent commit)"""
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from pram_amd import ops  # noqa: E402
from pram_amd.localization import candidates as cd  # noqa: E402
from pram_amd.localization.pose import localize_candidates  # noqa: E402
from pram_amd.nets.gml import GML  # noqa: E402
from tests import cand_ref as CR, helpers as H  # noqa: E402

B, SEG_K, MIN_KPTS, NQ, N_MAPS, LM = 16, 5, 32, 2048, 7, 28
N_CLASS = 1 + N_MAPS * LM
PLAN_LAUNCHES = 200


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    single = "--single" in sys.argv
    dev = torch.device("cuda:0")
    maps = [CR.make_map(41 + i, start_sid=LM * i) for i in range(1 if single else N_MAPS)]
    a = maps[0]
    nf = len(a["frames"])
    qs = []
    for b in range(B):
        f = 2 + b % (nf - 4)
        qs.append(CR.make_query(50 + b, a, [(2 * f, 260), (2 * f + 1, 200), (2 * f + 2, 260), (2 * ((f + 3) % nf), 260), (2 * ((f + 5) % nf) + 1, 200),
                                            (None, NQ - 1180)], NQ, N_CLASS))
    build = lambda m: cd.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], m["start_sid"])
    stores = {"ReferenceStore(A)": cd.ReferenceStore(a["frames"], a["seg_ref_frame_ids"], 0, device=dev)}
    if not single:
        from pram_amd.localization.multimap import MultiMapStore
        stores["MultiMapStore([A])"] = MultiMapStore([build(a)], ["A"], device=dev)
        stores[f"MultiMapStore of {N_MAPS} maps"] = MultiMapStore([build(m) for m in maps], [f"map{i}" for i in range(N_MAPS)], device=dev)
    feats, seg = CR.batch_features(qs, dev)
    cams = [("PINHOLE", 640, 480, [505.0, 498.0, 322.0, 237.0])] * B
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    kw = dict(seg_k=SEG_K, min_kpts=MIN_KPTS, threshold=4.0, min_inliers=30)
    with ops.guard_scope("deferred"):
        vote = cd.vote_candidates(feats, seg, SEG_K)
        counts = feats["counts"].contiguous()

        def plans(store):
            t = store.tables(dev)
            for _ in range(PLAN_LAUNCHES):
                ops.cand_plan(vote["win_sid"], vote["win_count"], vote["n_win"], vote["seg_ids"], counts, N_CLASS, t, MIN_KPTS, 0.5, True)

        calls = {name: (lambda s=s: localize_candidates(feats, seg, s, net, cams, **kw)) for name, s in stores.items()}
        first = {name: fn() for name, fn in calls.items()}
        for _ in range(2):
            for name, fn in calls.items():
                fn(), plans(stores[name])
        torch.cuda.synchronize()
        t_call, t_plan = {n: [] for n in calls}, {n: [] for n in calls}
        for _ in range(reps):
            for name, fn in calls.items():
                t_call[name].append(timed(fn))
            for name in calls:
                t_plan[name].append(timed(lambda: plans(stores[name])) / PLAN_LAUNCHES)
    med = statistics.median
    base = med(t_call["ReferenceStore(A)"])
    pairs = [(c["n_query_kpts"], c["n_ref_kpts"], c["semantic_matching"]) for r in first["ReferenceStore(A)"] for c in r["candidates"]]
    print(f"pairs {len(pairs)}, semantic {sum(p[2] for p in pairs)}, query side {min(p[0] for p in pairs)}..{max(p[0] for p in pairs)}, "
          f"reference side {min(p[1] for p in pairs)}..{max(p[1] for p in pairs)}, classes {N_CLASS}, reps {reps}")
    for name in calls:
        same = all(ca["sid"] == cb["sid"] and ca["n_ref_kpts"] == cb["n_ref_kpts"] and torch.equal(ca["matches0"], cb["matches0"])
                   for ra, rb in zip(first[name], first["ReferenceStore(A)"]) for ca, cb in zip(ra["candidates"], rb["candidates"]))
        t = t_call[name]
        print(f"localize_candidates, {name}: median {med(t):.3f} ms, min {min(t):.3f}, max {max(t):.3f}, ratio to ReferenceStore(A) {med(t) / base:.4f}, "
              f"matches0 equal to ReferenceStore(A)'s: {same}")
    for name in calls:
        t = t_plan[name]
        entry = "pram_cand_plan_maps" if "lm_start" in stores[name].tables(dev) else "pram_cand_plan"
        print(f"{entry} alone ({PLAN_LAUNCHES} back-to-back launches, per launch), {name}: median {1000 * med(t):.2f} us, min {1000 * min(t):.2f}, max {1000 * max(t):.2f}")


if __name__ == "__main__":
    main()
