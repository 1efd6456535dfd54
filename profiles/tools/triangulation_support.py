"""What stage 2b of the triangulation (min_support of triangulate_map: a match stays only when observations in third frames agree
with it) does to a simulated map: tests/triangulation_support_ref.py's sweep_scene at 2000 points and 30 frames, wrong matches at
several shares of the true ones, all of them on the epipolar line; writes profiles/triangulation_support.md.

    python profiles/tools/triangulation_support.py [--points 2000] [--frames 30] [--shares 0,0.01,0.02,0.05,0.1] [--seed 1] [--out FILE]

The support counts come from the numpy restatement (CPU) and from the device and have to be equal, edge by edge, or nothing is
written; components, tracks and points are the device's (build_tracks, triangulate_tracks)."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

NEAR = 0.01      # the scene's unit is the metre: cameras on a ring of radius 9 around points in a box of side 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--shares", default="0,0.01,0.02,0.05,0.1")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulation_support.md"))
    a = ap.parse_args()
    import torch
    from pram_amd.localization import triangulation as TG
    from tests import triangulation_ref as TR
    from tests import triangulation_support_ref as SR
    assert torch.cuda.is_available(), "the sweep needs the GPU: the device's counts are half of it"
    dev = torch.device("cuda:0")
    rows = []
    for p in [float(x) for x in a.shares.split(",")]:
        t0 = time.perf_counter()
        s = SR.sweep_scene(p, a.seed, n_points=a.points, n_frames=a.frames)
        table = TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), dev)
        v = TG.verify_matches(table, s["pairs"], s["matches"])
        e = np.concatenate([s["frame_off"][s["pairs"][i]] + k for i, k in zip(v["pair_index"].tolist(), v["kept"])])
        true = s["owner"][e[:, 0]] == s["owner"][e[:, 1]]
        assert len(e) == s["n_true"] + s["n_wrong"] and int((~true).sum()) == s["n_wrong"], "a planted match failed verification"
        ref = SR.support(s, e)
        print(f"p = {p}: {len(e)} edges, {s['n_wrong']} wrong, scene and restatement in {time.perf_counter() - t0:.1f} s", flush=True)
        for ms in (0, 1, 2):
            keep = np.ones(len(e), dtype=bool)
            if ms:
                got = TG.support_matches(table, e, min_support=ms)
                assert np.array_equal(got["support"], ref["support"]), "the device's counts differ from the restatement's"
                keep = got["keep"]
            trk = TG.build_tracks(table, np.where(keep[:, None], e, -1))
            tri = TG.triangulate_tracks(table, trk)
            xyz = tri["xyz"][tri["accept"]]
            d = np.linalg.norm(xyz[:, None, :] - s["xyz"][None, :, :], axis=2) if len(xyz) else np.zeros((0, a.points))
            near = d.min(1) <= NEAR
            sizes = np.diff(trk["trk_off"])
            rows.append((p, ms, len(e), s["n_wrong"], len(sizes), int(sizes.max(initial=0)), int((TG.track_conflicts(trk) > 0).sum()), int(tri["accept"].sum()),
                         int(near.sum()), len(set(d.argmin(1)[near].tolist())), int((true & ~keep).sum()), int((~true & keep).sum())))
            print("   ", rows[-1], flush=True)
    lines = ["# Triangulation, stage 2b: what third-view support does to a simulated map", "",
             f"Written by `python profiles/tools/triangulation_support.py --points {a.points} --frames {a.frames} --shares {a.shares} --seed {a.seed}`.", "",
             f"tests/triangulation_support_ref.py's sweep_scene: {a.frames} frames on a ring of radius 9 over the five camera models, {a.points} points in a box of",
             f"side 2, each seen in 4 to 9 consecutive frames, pairs up to 3 frames apart, keypoint noise uniform in +-{TR.NOISE} px, every true match",
             "present.  Wrong matches are a share p of the true ones, drawn among keypoint pairs of two different points whose epipolar errors",
             "are both below 3 px: every one of them passes verification (asserted).  The support counts of the numpy restatement and of the",
             "device were equal on every edge of every row below (asserted); components, tracks and points are the device's.  A component is",
             "a track of two rows or more and yields one point at most.  `near` counts the accepted points within 1 cm of a planted point",
             "(the scene's unit read as the metre), `distinct` the different planted points among them; a conflicting track holds two",
             "entries of one frame (track_conflicts > 0).", "",
             "| p | min_support | edges | wrong | components | largest | conflicting | accepted | near | distinct | true edges dropped | wrong edges kept |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    lines += ["| " + " | ".join([f"{r[0] * 100:g} %"] + [str(x) for x in r[1:]]) + " |" for r in rows]
    lines += [""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    old = Path(a.out).read_text() if Path(a.out).exists() else ""
    if "## Reading" in old:      # written by hand below the tables: carried over, to be read again against the new numbers
        lines += [old[old.index("## Reading"):]]
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
