"""Writes tests/golden/mapbuild_sweep_pinned.npz: what the REFERENCE's RecMap.create_virtual_frame_3 (recognition/recmap.py) produces
on the sweep scenes of tests/mapbuild_ref.py whose gain_floor is the 0.01 the reference hard-codes (MR.SWEEP_PINNED) — the frame
indices of seg_ref[sid][*] and their counts, nothing else.  tests/golden/mapbuild_pinned.npz is not touched.

Needs the reference tree beside the repository, with the import shims and stand-ins of tests/tools/gen_mapbuild_pinned.py; never
runs in the test suite.

    python tests/tools/gen_mapbuild_sweep_pinned.py
"""
from __future__ import annotations

import contextlib
import io
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import gen_golden as G  # noqa: E402
from tests import mapbuild_ref as MR  # noqa: E402


def run_reference(ref, s: dict):
    F, p = s["F"], s["params"]
    name = lambda f: ("ign" if s["ignored"][f] else "seq") + f"/frame_{f:03d}.jpg"
    images = {MR.FRAME_ID0 + f: SimpleNamespace(name=name(f), qvec=s["cams"][f, 0:4].copy(), tvec=s["cams"][f, 4:7].copy(), camera_id=f,
                                                point3D_ids=s["frame_point_ids"][f].copy()) for f in range(F)}
    cameras = {f: SimpleNamespace(model="PINHOLE", params=s["cams"][f, 7:11].copy(), width=int(s["cams"][f, 11]), height=int(s["cams"][f, 12]))
               for f in range(F)}
    points3D = {int(q): SimpleNamespace(id=int(q), xyz=s["xyz"][q], image_ids=[MR.FRAME_ID0 + f for f in v]) for q, v in s["point_frames"].items()}
    rm = ref.RecMap.__new__(ref.RecMap)
    rm.cameras, rm.images, rm.points3D = cameras, images, points3D
    rm.seg_p3d = {sid: [int(q) for q in pts] for sid, pts in enumerate(s["landmarks"])}
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        rm.create_virtual_frame_3(save_fn=str(Path(tmp) / "vrf.npy"), save_vrf_dir=None, show_time=-1, ignored_cameras=["ign"],
                                  min_cover_ratio=p["min_cover_ratio"], min_obs=p["min_obs"], topk_imgs=p["topk_imgs"], n_vrf=p["n_vrf"],
                                  image_root="")
        seg_ref = np.load(str(Path(tmp) / "vrf.npy"), allow_pickle=True)[()]
    vrf = np.full((len(s["landmarks"]), p["n_vrf"]), -1, dtype=np.int32)
    n = np.zeros(len(s["landmarks"]), dtype=np.int32)
    for sid in range(len(s["landmarks"])):
        ids = [seg_ref[sid][k]["image_id"] - MR.FRAME_ID0 for k in sorted(seg_ref[sid].keys())]
        vrf[sid, :len(ids)], n[sid] = ids, len(ids)
    return vrf, n


def main():
    G.import_reference()
    G._stub_missing_modules()
    import recognition.recmap as ref
    ref.cv2.imread = lambda path: np.zeros((MR.HEIGHT, MR.WIDTH, 3), dtype=np.uint8)
    ref.cv2.waitKey = lambda t: -1
    ref.plot_kpts = lambda img, **kw: img
    out = {"seed": MR.SEED}
    for name in MR.SWEEP_PINNED:
        s = MR.sweep_scene(name, MR.SEED)
        assert s["params"]["gain_floor"] == 0.01, name
        t = time.time()
        vrf, n = run_reference(ref, s)
        differ = [l for l, want in enumerate(s["vrf"]) if vrf[l, :n[l]].tolist() != want]
        print(f"  {name}: {len(s['landmarks'])} landmarks in {time.time() - t:.1f} s, the restatement differs on {differ}")
        out[name + "_vrf"], out[name + "_vrf_n"] = vrf, n
    G.save("mapbuild_sweep_pinned", **out)


if __name__ == "__main__":
    main()
