"""Writes tests/golden/compress_pinned.npz: what the REFERENCE's RecMap.compress_map_by_projection_v2 (recognition/recmap.py) writes
on tests/compress_ref.py::scene for the three configurations of compress_ref.CONFIGS — the retained images in order, every image's
point list and every point's image list, read back from its images.bin / points3D.bin with the reference's read_compressed_model —
and the keypoints RefFrame.associate_keypoints_with_point3Ds (localization/refframe.py) gives two of the retained frames.

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are); never runs in
the test suite.  open3d, sklearn, h5py and cv2 are stand-ins and the RecMap object is built with __new__, as in
gen_mapbuild_pinned.py.  The fixture holds results only: ids, orders and projected keypoints.

The reference alone has to be unambiguous on the scene, so compress_ref.check_scene is asserted first: pairwise distinct
covisibility counts in every reference frame's list (the reference's order comes from an unstable argsort otherwise), and every
decision further than 1e-6 from its threshold (the reference's BLAS products round differently from the restatement's written-out
sums, by about 1e-12 at these magnitudes).  Re-draw compress_ref.SEED until it passes.

    python tests/tools/gen_compress_pinned.py
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
from tests import compress_ref as CR  # noqa: E402

ASSOC_FRAMES = (2, 13)      # a reference frame and a frame retained in part, both of configuration c30


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in lists])
    return off, (np.concatenate([np.asarray(v, dtype=np.int32) for v in lists]) if len(lists) else np.zeros(0, dtype=np.int32))


def main():
    G.import_reference()
    G._stub_missing_modules()
    import recognition.recmap as ref
    import localization.refframe as ref_frame
    from colmap_utils.read_write_model import read_compressed_model
    s = CR.scene(CR.SEED)
    CR.check_scene(s)
    off = s["frame_off"]
    images = {CR.FRAME_ID0 + f: SimpleNamespace(id=CR.FRAME_ID0 + f, name=f"seq/frame_{f:02d}.jpg", qvec=s["cams"][f, 0:4].copy(),
                                                tvec=s["cams"][f, 4:7].copy(), camera_id=1, xys=s["xys"][off[f]:off[f + 1]].copy(),
                                                point3D_ids=s["point3D_ids"][off[f]:off[f + 1]].copy()) for f in range(CR.F)}
    from colmap_utils.read_write_model import Camera as RefCamera
    cameras = {1: RefCamera(id=1, model="PINHOLE", width=CR.WIDTH, height=CR.HEIGHT, params=np.array(CR.INTRINSICS))}
    points3D = {int(p): SimpleNamespace(id=int(p), xyz=s["pt_xyz"][i].copy(), rgb=np.array([1, 2, 3]), error=float(s["pt_err"][i]),
                                        image_ids=np.array([CR.FRAME_ID0 + f for f in s["point_frames"][int(p)]]),
                                        point2D_idxs=np.zeros(int(s["pt_obs"][i]), dtype=np.int64)) for i, p in enumerate(s["pt_ids"].tolist())}
    rm = ref.RecMap.__new__(ref.RecMap)
    rm.cameras, rm.images, rm.points3D = cameras, images, points3D
    vrf = {sid: {vi: {"image_id": CR.FRAME_ID0 + f, "original_points3d": []} for vi, f in enumerate(fs)} for sid, fs in s["seg_ref"].items()}
    out = {"seed": CR.SEED}
    models = {}
    for tag, cfg in CR.CONFIGS.items():
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            np.save(str(Path(tmp) / "vrf.npy"), vrf)
            np.save(str(Path(tmp) / "point3D_desc.npy"), {p: np.zeros(1, dtype=np.float32) for p in points3D})
            rm.compress_map_by_projection_v2(vrf_path=str(Path(tmp) / "vrf.npy"), point3d_desc_path=str(Path(tmp) / "point3D_desc.npy"), vrf_frames=1,
                                             covisible_frames=cfg["covisible_frames"], radius=CR.RADIUS, nkpts=cfg["nkpts"],
                                             save_dir=str(Path(tmp) / "compress"))
            _, r_images, r_points = read_compressed_model(str(Path(tmp) / "compress"), ".bin")
        models[tag] = (r_images, r_points)
        frames = [fid - CR.FRAME_ID0 for fid in r_images]      # the file's order is the dict's: the retained order
        out[tag + "_frames"] = np.array(frames, dtype=np.int32)
        out[tag + "_list_off"], out[tag + "_list_ids"] = csr([r_images[fid].point3D_ids for fid in r_images])
        out[tag + "_pt_ids"] = np.array(list(r_points), dtype=np.int32)
        out[tag + "_pt_off"], pf = csr([r_points[p].image_ids for p in r_points])
        out[tag + "_pt_frames"] = (pf - CR.FRAME_ID0).astype(np.int32)
        mine = s["results"][tag]
        same = frames == mine["frames"] and all(np.array_equal(r_images[CR.FRAME_ID0 + f].point3D_ids, mine["lists"][f]) for f in frames) and \
            list(r_points) == list(mine["point_frames"]) and all((r_points[p].image_ids - CR.FRAME_ID0).tolist() == mine["point_frames"][p] for p in r_points)
        print(f"  {tag}: {len(frames)} frames {frames}, {len(r_points)} points; the restatement {'agrees' if same else 'DIFFERS'}")
    # ---- associate_keypoints_with_point3Ds on two retained frames of c30, against the compressed map's points
    r_images, r_points = models["c30"]
    at = {int(p): i for i, p in enumerate(s["pt_ids"].tolist())}
    p3ds = {p: SimpleNamespace(xyz=r_points[p].xyz, descriptor=np.zeros(1, dtype=np.float32), error=float(s["pt_err"][at[p]]), seg_id=int(s["pt_sid"][at[p]]))
            for p in r_points}
    for f in ASSOC_FRAMES:
        img = r_images[CR.FRAME_ID0 + f]
        rf = ref_frame.RefFrame.__new__(ref_frame.RefFrame)
        rf.camera, rf.qvec, rf.tvec, rf.point3D_ids = cameras[1], img.qvec, img.tvec, img.point3D_ids
        assert rf.associate_keypoints_with_point3Ds(point3Ds=p3ds)
        out[f"assoc_{f}_keypoints"], out[f"assoc_{f}_ids"] = rf.keypoints.astype(np.float64), rf.point3D_ids.astype(np.int32)
        mine = CR.frame_rows(s, f, rf.point3D_ids)
        print(f"  frame {f}: {len(rf.point3D_ids)} keypoints, |reference - restatement| <= {np.abs(rf.keypoints - mine['keypoints']).max():.2e}")
    out["assoc_frames"] = np.array(ASSOC_FRAMES, dtype=np.int32)
    G.save("compress_pinned", **out)


if __name__ == "__main__":
    main()
