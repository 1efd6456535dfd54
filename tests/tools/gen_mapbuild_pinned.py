"""Writes tests/golden/mapbuild_pinned.npz: what the REFERENCE's RecMap.assign_point3D_descriptor and RecMap.create_virtual_frame_3
(recognition/recmap.py) produce on tests/mapbuild_ref.py::scene — the chosen track position of about 300 points, and the image ids
of seg_ref[sid][*] on the 8 landmarks.

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are); never runs in
the test suite.  open3d, sklearn, h5py and cv2 are stand-ins: the object is built with __new__, the feature file is a dict of
arrays (an ndarray answers [()]), imread answers a blank image, waitKey -1, plot_kpts hands its image back.  Both methods only
save their result, so each writes into a temporary directory that is read back.  The fixture holds results only.  The descriptor
choices depend on the machine's fp32 BLAS; tests/test_mapbuild_cpu.py compares them through a derived gap for that reason.

    python tests/tools/gen_mapbuild_pinned.py
"""
from __future__ import annotations

import contextlib
import io
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import gen_golden as G  # noqa: E402
from tests import mapbuild_ref as MR  # noqa: E402

N_RANDOM = 280


def pinned_points(s: dict) -> list:
    """The named tracks whose every index is in range (the reference raises on the others) and the first N_RANDOM drawn ones."""
    named = [p for k, p in s["special"].items() if k not in ("dropped_short", "dropped_long", "all_dropped")]
    first = min(p for k, p in s["special"].items() if k.startswith("len"))
    drawn = [p for p in s["point_ids"].tolist() if p >= first and p not in set(s["special"].values())][:N_RANDOM]
    return sorted(named + drawn)


def main():
    G.import_reference()
    G._stub_missing_modules()
    import recognition.recmap as ref
    s = MR.scene(MR.SEED)
    name = lambda f: ("ign" if s["ignored"][f] else "seq") + f"/frame_{f:02d}.jpg"
    images = {MR.FRAME_ID0 + f: SimpleNamespace(name=name(f), qvec=s["cams"][f, 0:4].copy(), tvec=s["cams"][f, 4:7].copy(), camera_id=f,
                                                point3D_ids=s["frames"][f]["point3D_ids"].copy()) for f in range(MR.F)}
    cameras = {f: SimpleNamespace(model="PINHOLE", params=s["cams"][f, 7:11].copy(), width=int(s["cams"][f, 11]), height=int(s["cams"][f, 12]))
               for f in range(MR.F)}
    points3D = {int(p): SimpleNamespace(id=int(p), xyz=s["xyz"][int(p)], image_ids=im.tolist(), point2D_idxs=kp.tolist())
                for p, (im, kp) in s["tracks"].items()}
    rm = ref.RecMap.__new__(ref.RecMap)
    rm.cameras, rm.images = cameras, images
    out = {"seed": MR.SEED}

    # ---- assign_point3D_descriptor on the pinned tracks
    pids = pinned_points(s)
    rm.points3D = {p: points3D[p] for p in pids}
    feat = {images[MR.FRAME_ID0 + f].name: {"descriptors": np.ascontiguousarray(s["frames"][f]["descriptors"].transpose())} for f in range(MR.F)}
    ref.h5py.File = lambda fn, mode="r": feat
    ref.tqdm = lambda it, **kw: it
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        rm.assign_point3D_descriptor(feature_fn="features.h5", save_fn=str(Path(tmp) / "desc.npy"), n_process=1)
        got = np.load(str(Path(tmp) / "desc.npy"), allow_pickle=True)[()]
    choice = []
    rows = MR.entry_rows(s["frame_off"].astype(np.int64), s["trk_frame"], s["trk_kpt"])
    for p in pids:
        i = s["index_of_point"][p]
        e = rows[s["trk_off"][i]:s["trk_off"][i + 1]]
        same = [t for t in range(len(e)) if e[t] >= 0 and np.array_equal(s["descriptors"][e[t]].view(np.uint32), np.asarray(got[p]).view(np.uint32))]
        assert same, p
        choice.append(same[0])      # a repeated row: the lowest position that holds it
    out["desc_point_ids"], out["desc_choice"] = np.array(pids, dtype=np.int64), np.array(choice, dtype=np.int32)
    agree = int(sum(c == s["choice"][s["index_of_point"][p]] for p, c in zip(pids, choice)))
    print(f"  descriptors: {len(pids)} tracks, {agree} choices equal the float64 restatement's")

    # ---- create_virtual_frame_3 on the 8 landmarks
    rm.points3D = points3D
    rm.seg_p3d = {sid: [int(p) for p in pts] for sid, pts in enumerate(s["landmarks"])}
    ref.cv2.imread = lambda path: np.zeros((MR.HEIGHT, MR.WIDTH, 3), dtype=np.uint8)
    ref.cv2.waitKey = lambda t: -1
    ref.plot_kpts = lambda img, **kw: img
    p = MR.VRF_PARAMS
    ignored = ["ign"]
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        rm.create_virtual_frame_3(save_fn=str(Path(tmp) / "vrf.npy"), save_vrf_dir=None, show_time=-1, ignored_cameras=ignored,
                                  min_cover_ratio=p["min_cover_ratio"], min_obs=p["min_obs"], topk_imgs=p["topk_imgs"], n_vrf=p["n_vrf"],
                                  image_root="")
        seg_ref = np.load(str(Path(tmp) / "vrf.npy"), allow_pickle=True)[()]
    vrf = np.full((len(s["landmarks"]), p["n_vrf"]), -1, dtype=np.int32)
    n = np.zeros(len(s["landmarks"]), dtype=np.int32)
    for sid in range(len(s["landmarks"])):
        ids = [seg_ref[sid][k]["image_id"] - MR.FRAME_ID0 for k in sorted(seg_ref[sid].keys())]
        vrf[sid, :len(ids)], n[sid] = ids, len(ids)
        print(f"  landmark {sid}: frames {ids}" + ("" if ids == s["vrf"][sid] else f"  (restatement: {s['vrf'][sid]})"))
    out["vrf"], out["vrf_n"] = vrf, n
    G.save("mapbuild_pinned", **out)


if __name__ == "__main__":
    main()
