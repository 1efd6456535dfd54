"""What the triangulation's further rounds (split_rounds of triangulate_map: the entries that fell out of accepted tracks are
grouped and solved again) recover on a simulated map, and what a round costs: tests/triangulation_support_ref.py's sweep_scene at
2000 points and 30 frames, wrong matches at several shares of the true ones, all of them on the epipolar line; writes
profiles/triangulation_split.md.

    python profiles/tools/triangulation_split.py [--points 2000] [--frames 30] [--shares 0,0.01,0.02,0.05,0.1] [--seed 1] [--out FILE]

Everything is the device's (verify_matches, support_matches, build_tracks, triangulate_tracks, split_edges run round after round,
so that every round's table can be looked at); the points of those stages are asserted to be triangulate_map's.  The times are of
the device-resident path (triangulate_map's own calls), every stage closed by a synchronisation, the median of --repeat runs."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

NEAR = 0.01      # the scene's unit is the metre: cameras on a ring of radius 9 around points in a box of side 2
ROUNDS = (0, 1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--shares", default="0,0.01,0.02,0.05,0.1")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulation_split.md"))
    a = ap.parse_args()
    import torch
    from pram_amd.localization import triangulation as TG
    from tests import triangulation_ref as TR
    from tests import triangulation_support_ref as SR
    assert torch.cuda.is_available(), "the sweep needs the GPU"
    dev = torch.device("cuda:0")
    R = max(ROUNDS)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    rows, times = [], []
    for p in [float(x) for x in a.shares.split(",")]:
        t0 = time.perf_counter()
        s = SR.sweep_scene(p, a.seed, n_points=a.points, n_frames=a.frames)
        table = TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), dev)
        v = TG.verify_matches(table, s["pairs"], s["matches"])
        e = np.concatenate([s["frame_off"][s["pairs"][i]] + k for i, k in zip(v["pair_index"].tolist(), v["kept"])])
        assert len(e) == s["n_true"] + s["n_wrong"], "a planted match failed verification"
        print(f"p = {p}: {len(e)} edges, {s['n_wrong']} wrong, scene in {time.perf_counter() - t0:.1f} s", flush=True)
        for ms in (0, 1):
            edges = TG.support_matches(table, e, min_support=ms)["edges"] if ms else e
            # ---- the rounds by hand, each round's table and points on the host
            per_round, state, cur = [], None, edges
            for k in range(R + 1):
                trk = TG.build_tracks(table, cur)
                if len(trk["trk_label"]) == 0:
                    break
                tri = TG.triangulate_tracks(table, trk)
                xyz = tri["xyz"][tri["accept"]]
                d = np.linalg.norm(xyz[:, None, :] - s["xyz"][None, :, :], axis=2) if len(xyz) else np.zeros((0, a.points))
                near = d.min(1) <= NEAR if len(xyz) else np.zeros(0, dtype=bool)
                per_round.append({"tracks": len(trk["trk_label"]), "accepted": int(tri["accept"].sum()), "near": int(near.sum()),
                                  "found": set(d.argmin(1)[near].tolist()) if len(xyz) else set(), "conflicting": int((TG.track_conflicts(trk) > 0).sum()),
                                  "xyz": xyz})
                nxt = TG.split_edges(table, edges, trk, tri, state)
                state, cur = nxt["state"], nxt["edges"]
                if nxt["n_live"] == 0:
                    break
            for r in ROUNDS:
                m = TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev, min_support=ms, split_rounds=r)
                use = per_round[:r + 1]
                assert np.array_equal(m["point3D_xyzs"], np.concatenate([x["xyz"] for x in use])), "triangulate_map differs from the stages run by hand"
                found, distinct = set(), []
                for x in use:
                    found |= x["found"]
                    distinct.append(len(found))
                acc, near = sum(x["accepted"] for x in use), sum(x["near"] for x in use)
                rows.append((p, ms, r, len(use) - 1, " / ".join(str(x["accepted"]) for x in use), " / ".join(str(x["near"]) for x in use),
                             " / ".join(str(x) for x in distinct), " / ".join(str(x["conflicting"]) for x in use), acc - near))
                print("   ", rows[-1], flush=True)
            # ---- the time of every round, device-resident, beside round 0's stages 3 and 4
            p_ = {**TG.DEFAULTS, "min_support": ms}
            n_e = len(edges)
            e_dev = TG._up(TG._edges(edges), dev)
            runs = []
            for _ in range(a.repeat + 1):      # the first run warms up
                one, state = [], None
                t, t3 = timed(lambda: TG._tracks(table, e_dev, n_e))
                out, t4 = timed(lambda: TG._triangulate(table, t, p_))
                one.append((t3, t4, 0.0))
                for k in range(1, R + 1):
                    sp, tm = timed(lambda: TG._split(table, e_dev, n_e, t, out, state))
                    state = sp["state"]
                    if int(sp["n_live"].item()) == 0:
                        break
                    t, t3 = timed(lambda: TG._tracks(table, sp["edges"], n_e))
                    if t["n_tracks"] == 0:
                        break
                    out, t4 = timed(lambda: TG._triangulate(table, t, p_))
                    one.append((t3, t4, tm))
                runs.append(one)
            runs = np.array([r_ for r_ in runs[1:] if len(r_) == len(runs[1])])      # [repeat, rounds, 3]
            med, total = np.median(runs, axis=0), runs.sum(2)
            times.append((p, ms, med, total.min(0), total.max(0)))
            print("    ms per round (tracks, stage 4, split):", np.round(med, 3).tolist(), flush=True)
    lines = ["# Triangulation: what further rounds over the outliers recover, and what a round costs", "",
             f"Written by `python profiles/tools/triangulation_split.py --points {a.points} --frames {a.frames} --shares {a.shares} --seed {a.seed}`.", "",
             f"The scene and the shares of profiles/triangulation_support.md: tests/triangulation_support_ref.py's sweep_scene, {a.frames} frames on a",
             f"ring of radius 9 over the five camera models, {a.points} points in a box of side 2, each seen in 4 to 9 consecutive frames, pairs up",
             f"to 3 frames apart, keypoint noise uniform in +-{TR.NOISE} px, every true match present, wrong matches a share p of the true ones, all",
             "on the epipolar line (every one passes verification, asserted).  Everything is the device's; the points of the stages run by",
             "hand were bit-equal to triangulate_map's on every row (asserted).  `rounds run` is the number of further rounds that reached",
             "stage 4 (the rounds end sooner than `split_rounds` when no edge between FREE rows or no track is left).  Per round, round 0",
             "first: `accepted` tracks, those `near` (within 1 cm of) a planted point, the `distinct` planted points found so far (cumulative),",
             "and the `conflicting` tracks of the round's table (two entries of one frame).  `not near` counts the accepted points of all",
             "rounds that lie further than 1 cm from every planted point.", "",
             "| p | min_support | split_rounds | rounds run | accepted | near | distinct | conflicting | not near |", "|---|---|---|---|---|---|---|---|---|"]
    lines += ["| " + " | ".join([f"{r[0] * 100:g} %"] + [str(x) for x in r[1:]]) + " |" for r in rows]
    lines += ["", "## The time of a round", "",
              f"The same run on the same device: triangulate_map's own device-resident calls, each closed by a synchronisation, the median of {a.repeat}",
              "runs after a warm-up, in ms.  `tracks` is stage 3 (the components, with their reads of the done flag, and the track table with",
              "its read of the sizes), `stage 4` the solve, `split` the marking and the filter with the read of the count.  A round repeats the",
              "components over all rows, whatever is left.  `round total` is the sum of the three medians, `spread` the smallest and the",
              "largest total of a single run: these are windows of a millisecond and less, in which launches and reads weigh as much as",
              "the kernels.", "", "| p | min_support | round | tracks | stage 4 | split | round total | spread |", "|---|---|---|---|---|---|---|---|"]
    for p, ms, med, lo, hi in times:
        for k, (t3, t4, tm) in enumerate(med.tolist()):
            lines.append(f"| {p * 100:g} % | {ms} | {k} | {t3:.3f} | {t4:.3f} | {'' if k == 0 else f'{tm:.3f}'} | {t3 + t4 + tm:.3f} | {lo[k]:.3f} .. {hi[k]:.3f} |")
    lines += [""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    old = Path(a.out).read_text() if Path(a.out).exists() else ""
    if "## Reading" in old:      # written by hand below the tables: carried over, to be read again against the new numbers
        lines += [old[old.index("## Reading"):]]
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
