"""Map building on the device: the two inputs of a ReferenceStore that the reference computes offline on the CPU.

Reference: recognition/recmap.py.
  * RecMap.assign_point3D_descriptor (recmap.py:124-194): one descriptor per 3D point, the row of its track with the smallest
    median distance 2 - 2 <a_i, a_j> to the track's rows -> :func:`assign_point_descriptors`.
  * find_best_vrf_by_covisibility and the filter around it in RecMap.create_virtual_frame_3 (recmap.py:263-355, 369-403; read by
    SingleMap3D at singlemap3d.py:72-82): the virtual reference frames of every landmark, a greedy cover of the landmark's points
    by the frames observing them -> :func:`select_reference_frames`.
:func:`build_store_inputs` runs both and returns ``point3D_descriptors`` and ``seg_ref_frame_ids`` as ReferenceStore takes them.
The kernels are csrc/mapbuild.hip; torch here is plumbing (uploads, one read-back per stage).

Where this differs from the reference, on purpose:
  * arithmetic: the distances are float64 sums of the exact products of the fp32 descriptors, in one fixed order for every pair
    (the reference: an fp32 BLAS product, whose rounding depends on the machine).  The Gram matrix is therefore symmetric bit for
    bit, bit-identical rows get bit-identical medians, and a tie goes to the lowest track position — np.argmin's rule on a
    symmetric matrix.  Ties are common: the closest pair of a track of three always ties.
  * a track entry naming an image the map does not hold is dropped, as in the reference; an entry with a frame index out of range
    or a keypoint index outside its frame is dropped too (the reference would raise an IndexError).
  * a track with no entry left gets choice -1 and a zero descriptor (the reference raises on the empty array);
    build_store_inputs reports the choices beside the descriptors, so that a caller can tell such a point.
  * cameras: fx, fy, cx, cy as get_intrinsics_from_camera extracts them, no distortion (the reference's projection has none).
  * ``covisible_frame_ids`` and ``original_points3d`` of the reference's file are not produced: the store derives its own graph.
The k-means labelling that produces ``landmarks`` is localization/labelling.py; Birch labelling, Open3D outlier removal and
everything cv2 draws stay outside this repository; map compression, the next step of the reference's pipeline, is
localization/compress.py."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from pram_amd import ops

STORE_KEYS = ("seg_ref_frame_ids", "point3D_frame_ids", "point3D_xyzs", "point3D_descriptors")
DEFAULTS = dict(min_obs=120, topk_imgs=500, n_vrf=10, min_cover_ratio=0.9, gain_floor=0.01)      # create_virtual_frame_3's


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        from pram_amd._lib import PramHipError
        raise PramHipError("mapbuild: expected a CUDA device (pram_amd has no CPU path)")
    return device


def _csr(lists: Sequence, dtype) -> tuple:
    lens = np.fromiter((len(v) for v in lists), dtype=np.int64, count=len(lists))
    if lens.sum() >= 2 ** 31:
        raise ValueError("mapbuild: more than 2^31 - 1 entries")
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    flat = np.concatenate([np.asarray(v, dtype=dtype).reshape(-1) for v in lists]) if len(lists) and lens.sum() else np.zeros(0, dtype=dtype)
    return off, flat


def track_tables(store, tracks: Dict[int, tuple]) -> dict:
    """tracks: point id -> (image_ids, point2D_idxs), COLMAP's Point3D fields -> the CSR tables of the kernel on the host: point_ids
    int64 [P] ascending, trk_off int32 [P + 1], trk_frame int32 [E] (store frame index, -1 for an image the store does not hold),
    trk_kpt int32 [E]."""
    pids = np.array(sorted(int(k) for k in tracks.keys()), dtype=np.int64)
    imgs, kpts = [], []
    for p in pids.tolist():
        im, kp = tracks[p]
        im, kp = np.asarray(im).reshape(-1), np.asarray(kp).reshape(-1)
        if im.shape != kp.shape:
            raise ValueError(f"track of point {p}: {im.shape[0]} image ids, {kp.shape[0]} keypoint indices")
        imgs.append(im)
        kpts.append(kp)
    off, flat_img = _csr(imgs, np.int64)
    _, flat_kpt = _csr(kpts, np.int64)
    index_of = {fid: i for i, fid in enumerate(store.frame_ids)}
    frame = np.array([index_of.get(x, -1) for x in flat_img.tolist()], dtype=np.int32).reshape(-1)
    kpt = np.where((flat_kpt >= 0) & (flat_kpt < 2 ** 31), flat_kpt, -1).astype(np.int32)
    return {"point_ids": pids, "trk_off": off, "trk_frame": frame, "trk_kpt": kpt}


def _up(a: np.ndarray, device) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.shape[0] == 0:      # never an empty allocation behind a pointer
        a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
    return torch.from_numpy(a).to(device)


@torch.no_grad()
def assign_point_descriptors(store, tables: dict, device):
    """store: a ReferenceStore; tables: :func:`track_tables` (or the same arrays built otherwise) -> (pt_desc float32 [P, 128],
    pt_choice int32 [P]) on the device, aligned with tables["point_ids"]."""
    device = _device(device)
    t = store.tables(device)
    return ops.mapbuild_assign_descriptors(t, _up(tables["trk_off"], device), tables["trk_off"], _up(tables["trk_frame"], device),
                                           _up(tables["trk_kpt"], device))


def frame_cameras(frames: Sequence[dict]) -> np.ndarray:
    """[F, 13] float64: qvec (w, x, y, z), tvec, fx, fy, cx, cy, width, height of every frame dict (keys ``qvec``, ``tvec``,
    ``intrinsics`` = (fx, fy, cx, cy), ``width``, ``height``)."""
    out = np.zeros((len(frames), ops.MAPBUILD_CAM_COLS), dtype=np.float64)
    for i, f in enumerate(frames):
        missing = [k for k in ("qvec", "tvec", "intrinsics") if k not in f]
        if missing:
            raise ValueError(f"reference frame {i}: missing {missing}")
        out[i, 0:4] = np.asarray(f["qvec"], dtype=np.float64).reshape(4)
        out[i, 4:7] = np.asarray(f["tvec"], dtype=np.float64).reshape(3)
        out[i, 7:11] = np.asarray(f["intrinsics"], dtype=np.float64).reshape(4)
        out[i, 11], out[i, 12] = float(f["width"]), float(f["height"])
    return out


@torch.no_grad()
def select_reference_frames(store, landmarks, cams: np.ndarray, pt_xyz: np.ndarray, device, frame_ignored: Optional[Sequence] = None,
                            **params):
    """store: a ReferenceStore whose point table comes from COLMAP's image_ids (point3D_frame_ids); landmarks: landmark id -> point
    ids in the label file's order (a dict or a sequence); cams: :func:`frame_cameras`; pt_xyz float64 [n_points, 3] aligned with
    store.pt_ids -> (lm_vrf int32 [L, n_vrf], lm_vrf_n int32 [L]) on the host, rows in the order of ``landmarks``, store frame
    indices in pick order.  params: min_obs, topk_imgs, n_vrf, min_cover_ratio, gain_floor (DEFAULTS)."""
    device = _device(device)
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"select_reference_frames: unknown parameters {sorted(unknown)}")
    p = {**DEFAULTS, **params}
    lists = list(landmarks.values()) if isinstance(landmarks, dict) else list(landmarks)
    lm_off, lm_points = _csr(lists, np.int64)
    F = store.n_frames
    ignored = np.zeros(F, dtype=np.int32) if frame_ignored is None else np.asarray(frame_ignored).astype(bool).astype(np.int32).reshape(-1)
    cams, pt_xyz = np.asarray(cams, dtype=np.float64), np.asarray(pt_xyz, dtype=np.float64)
    if ignored.shape[0] != F or cams.shape != (F, ops.MAPBUILD_CAM_COLS) or pt_xyz.shape != (len(store.pt_ids), 3):
        raise ValueError("select_reference_frames: frame_ignored [F], cams [F, 13] and pt_xyz [n_points, 3] must match the store")
    t = store.tables(device)
    vrf, n = ops.mapbuild_select_frames(t, _up(pt_xyz, device), _up(lm_off, device), lm_off, _up(lm_points, device), _up(ignored, device),
                                        _up(cams, device), **p)
    both = torch.cat([vrf, n[:, None]], dim=1).cpu().numpy()      # the one read-back
    return both[:, :-1], both[:, -1]


@torch.no_grad()
def build_store_inputs(frames: Sequence[dict], tracks: Dict[int, tuple], landmarks: dict, point3D_xyzs: dict, device,
                       frame_ignored: Optional[Sequence] = None, **params) -> dict:
    """frames: the dicts ReferenceStore takes, each with ``qvec``, ``tvec`` and ``intrinsics`` besides; tracks: point id ->
    (image_ids, point2D_idxs); landmarks: in-map landmark id -> point ids; point3D_xyzs: point id -> xyz
    -> a dict with the STORE_KEYS, keyword arguments of ``ReferenceStore(frames, **{k: out[k] for k in STORE_KEYS})``, and
    ``point3D_choice`` (point id -> position of the chosen entry in its track, -1: nothing kept, a zero descriptor).
    seg_ref_frame_ids holds frame ids (not indices), entry [0] the landmark's reference frame; a landmark without a frame gets
    an empty list."""
    from pram_amd.localization.candidates import ReferenceStore
    device = _device(device)
    frame_lists = {int(k): np.asarray(v[0]).reshape(-1) for k, v in tracks.items()}
    base = ReferenceStore(frames, {}, point3D_frame_ids=frame_lists)      # rows, frame_off and the point table; no landmark yet
    tables = track_tables(base, tracks)
    pt_desc, pt_choice = assign_point_descriptors(base, tables, device)
    xyz_of = {int(k): np.asarray(v, dtype=np.float64).reshape(3) for k, v in point3D_xyzs.items()}
    missing = [int(p) for p in base.pt_ids.tolist() if int(p) not in xyz_of]
    if missing:
        raise ValueError(f"point3D_xyzs: {len(missing)} points of the tracks have no xyz, e.g. point id {missing[0]}")
    pt_xyz = np.array([xyz_of[int(p)] for p in base.pt_ids.tolist()], dtype=np.float64).reshape(-1, 3)
    vrf, n = select_reference_frames(base, landmarks, frame_cameras(frames), pt_xyz, device, frame_ignored, **params)
    desc, choice = pt_desc.cpu().numpy(), pt_choice.cpu().numpy()
    keys = list(landmarks.keys()) if isinstance(landmarks, dict) else list(range(len(landmarks)))
    return {
        "point3D_descriptors": {int(p): desc[i] for i, p in enumerate(tables["point_ids"].tolist())},
        "point3D_choice": {int(p): int(choice[i]) for i, p in enumerate(tables["point_ids"].tolist())},
        "seg_ref_frame_ids": {int(k): [base.frame_ids[f] for f in vrf[i, :n[i]].tolist()] for i, k in enumerate(keys)},
        "point3D_frame_ids": frame_lists,
        "point3D_xyzs": xyz_of,
    }
