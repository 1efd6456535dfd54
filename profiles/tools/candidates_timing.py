"""Timing of localization.candidates.match_candidates against the bench's way of preparing the same pairs.

B = 16 queries of 512 keypoints, seg_k = 5 (80 pairs) on the seeded synthetic map of tests/cand_ref.py.  Yardstick: what
bench.py::_segk_step does with the matcher today — the pairs' index lists built once on the host, the query side gathered by torch
fancy indexing, the reference side a resident padded tensor, one grouped produce_matches, no correspondence step.  Both paths are
timed with HIP events, warm, interleaved on one device; prints medians and the yardstick's own spread.
    python profiles/tools/candidates_timing.py [--reps 24] [--once]      (--once: a single public call, for a kernel trace)"""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from pram_amd import ops  # noqa: E402
from pram_amd.localization import candidates as cd  # noqa: E402
from pram_amd.nets.gml import GML  # noqa: E402
from tests import cand_ref as CR, helpers as H  # noqa: E402

B, SEG_K, MIN_KPTS, NQ = 16, 5, 32, 512


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 24
    dev = torch.device("cuda:0")
    m = CR.make_map(41)
    nf = len(m["frames"])
    qs = []
    for b in range(B):
        f = 2 + b % (nf - 4)
        qs.append(CR.make_query(50 + b, m, [(2 * f, 200), (2 * f + 1, 150), (2 * f + 2, 60), (2 * ((f + 3) % nf), 40), (2 * ((f + 5) % nf) + 1, 20),
                                           (None, 42)], NQ, CR.N_CLASS))
    store = cd.ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, device=dev)
    feats, seg = CR.batch_features(qs, dev)
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    kw = dict(seg_k=SEG_K, min_kpts=MIN_KPTS)

    def ours():
        return cd.match_candidates(feats, seg, store, net, **kw)

    with ops.guard_scope("deferred"):
        out = ours()
        torch.cuda.synchronize()
        if "--once" in sys.argv:
            ours()
            torch.cuda.synchronize()
            return
        # the same 80 pairs, prepared the bench's way (built once, untimed)
        data = cd.gather_candidates(feats, cd.plan_candidates(feats, seg, store, **kw), store)
        host = dict(zip(ops.CAND_PLAN_FIELDS, data["plan_host"]))
        P = B * SEG_K
        M, N = int(host["lens0"].max()), int(host["lens1"].max())
        tok = cd.vote_candidates(feats, seg, SEG_K)["tokens"].cpu().numpy()
        idx = np.zeros((P, M), dtype=np.int64)
        for p in range(P):
            l0 = host["lens0"][p]
            idx[p, :l0] = np.arange(l0) if host["tok_off"][p] < 0 else tok[p // SEG_K, p % SEG_K, :l0]
        sk_q = torch.arange(B, device=dev).repeat_interleave(SEG_K)
        sk_idx = torch.from_numpy(idx).to(dev)
        ref = {k: data[k + "1"][:, :N].contiguous().clone() for k in ("descriptors", "norm_keypoints", "scores")}
        lens0, lens1 = data["lens0"].clone(), data["lens1"].clone()

        def yardstick():
            sub = lambda t: t[sk_q[:, None], sk_idx]
            d = {"descriptors0": sub(feats["descriptors"]), "keypoints0": sub(feats["keypoints"]), "scores0": sub(feats["scores"]), "lens0": lens0,
                 "image_shape0": (1, 3, 640, 480), "descriptors1": ref["descriptors"], "keypoints1": ref["norm_keypoints"], "scores1": ref["scores"],
                 "lens1": lens1, "image_shape1": (1, 3, 640, 480)}
            return net.produce_matches(d)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        for _ in range(3):
            yardstick(), ours()
        torch.cuda.synchronize()
        t_y, t_o = [], []
        for _ in range(reps):
            t_y.append(timed(yardstick))
            t_o.append(timed(ours))
    med = statistics.median
    live = int((host["frame"] >= 0).sum())
    print(f"pairs {P} (live {live}), query side {int(host['lens0'].min())}..{M}, reference side {int(host['lens1'].min())}..{N}, "
          f"semantic pairs {int(host['semantic'].sum())}, matches {sum(int(c['n_matches']) for q in out for c in q)}")
    print(f"yardstick (torch gather + produce_matches): median {med(t_y):.3f} ms, min {min(t_y):.3f}, max {max(t_y):.3f}, "
          f"spread (max - min) / median {100 * (max(t_y) - min(t_y)) / med(t_y):.1f} %, n = {len(t_y)}")
    print(f"match_candidates (vote + plan + gather + produce_matches + correspond): median {med(t_o):.3f} ms, min {min(t_o):.3f}, "
          f"max {max(t_o):.3f}, n = {len(t_o)}")
    print(f"ratio of medians ours / yardstick: {med(t_o) / med(t_y):.4f}")


if __name__ == "__main__":
    main()
