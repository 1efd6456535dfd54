"""Writes tests/golden/refine_matching_pinned.npz: what the REFERENCE's build_covisibility_graph, find_reference_frames and
refine_pose_by_matching (localization/singlemap3d.py) produce on tests/refine_ref.py::covisible_scene.

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are); never runs in
the test suite.  The reference object is built with __new__, the network is replaced by refine_ref's numpy mutual-nearest-neighbour
matcher and pycolmap's solver by a recorder that keeps what it is handed and answers with a fixed inlier pattern (every row whose
index is not a multiple of 3).  The fixture holds results only: the graph lists, the keypoint / point ids / landmarks the solver's
rows carry, and the frames of the vote.  The scene regenerates from the seed.

    python tests/tools/gen_refine_pinned.py
"""
from __future__ import annotations

import contextlib
import io
import sys
from pathlib import Path
from types import SimpleNamespace
from unittest import mock

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import gen_golden as G  # noqa: E402
from tests import refine_ref as RR  # noqa: E402

SEED, MIN_SIM = 7, 0.7
# (query, frame id the localisation kept, tracking status)
CASES = ((0, 101, 1), (1, 105, 1), (2, 107, 0), (3, 107, 1), (1, 104, 0), (0, 100, 1))


def inlier_pattern(n: int) -> np.ndarray:
    return np.arange(n) % 3 != 0


def main():
    G.import_reference()
    G._stub_missing_modules()
    import localization.singlemap3d as ref_sm
    from localization.refframe import RefFrame
    map_, queries, _ = RR.covisible_scene(SEED)
    ids = RR.frame_ids(map_)
    pf = RR.point_frames(map_)
    seg_of = {}
    for f in map_["frames"]:
        for pid, s in zip(f["point3D_ids"].tolist(), f["keypoint_segs"].tolist()):
            seg_of[pid] = s
    xyz_of = {}
    for f in map_["frames"]:
        for pid, x in zip(f["point3D_ids"].tolist(), f["xyzs"]):
            xyz_of.setdefault(pid, x)
    sm = ref_sm.SingleMap3D.__new__(ref_sm.SingleMap3D)
    sm.point3Ds = {pid: SimpleNamespace(xyz=xyz_of[pid], seg_id=seg_of[pid], frame_ids=np.array(fr)) for pid, fr in pf.items()}
    sm.reference_frames = {}
    for fid, f in zip(ids, map_["frames"]):
        rf = RefFrame.__new__(RefFrame)
        rf.id, rf.camera = fid, SimpleNamespace(width=f["width"], height=f["height"])
        rf.point3D_ids, rf.keypoints, rf.descriptors, rf.xyzs, rf.keypoint_segs = f["point3D_ids"], f["keypoints"], f["descriptors"], f["xyzs"], f["keypoint_segs"]
        sm.reference_frames[fid] = rf
    sm.config = {"localization": {"threshold": 12, "covisibility_frame": RR.COVIS}}
    mnn = RR.mnn_matcher(MIN_SIM)
    sm.matcher = lambda d: {"matches0": torch.from_numpy(mnn({k: (v[0].numpy() if torch.is_tensor(v) else v) for k, v in d.items()}))[None]}
    sm.build_covisibility_graph(frame_ids=RR.vrf_frame_ids(map_), n_frame=RR.COVIS)
    keys = sorted(sm.covisible_graph)
    lists = np.full((len(keys), RR.COVIS), -1, dtype=np.int64)
    for i, fid in enumerate(keys):
        lst = [int(x) for x in sm.covisible_graph[fid]]
        lists[i, :len(lst)] = lst
    want = RR.covisibility_graph(map_, RR.COVIS)
    assert all(want[fid] == lists[i][lists[i] >= 0].tolist() for i, fid in enumerate(keys)), "the restatement's graph differs"
    handed = {}

    def solver(pts2d, pts3d, camera, estimation_options=None, refinement_options=None):
        handed.update(pts2d=np.array(pts2d), pts3d=np.array(pts3d))
        inl = inlier_pattern(len(pts2d))
        return {"num_inliers": int(inl.sum()), "inliers": inl, "cam_from_world": mock.MagicMock()}
    ref_sm.pycolmap.absolute_pose_estimation = solver
    out = {"seed": SEED, "min_sim": MIN_SIM, "covisibility_frame": RR.COVIS, "n_cases": len(CASES), "graph_keys": np.array(keys), "graph_lists": lists}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self        # harness shim: the generator runs without a GPU
    try:
        for i, (b, ref_id, tracked) in enumerate(CASES):
            q = queries[b]
            n = q["count"]
            kp3 = np.concatenate([q["keypoints"][:n], q["scores"][:n, None]], 1)
            cam = SimpleNamespace(width=q["width"], height=q["height"])
            with contextlib.redirect_stdout(io.StringIO()):
                first = sm.match(query_data={"keypoints": kp3[:, :2], "scores": kp3[:, 2], "descriptors": q["descriptors"][:n], "camera": cam},
                                 ref_data=sm.reference_frames[ref_id].get_keypoints())
                q_frame = SimpleNamespace(reference_frame_id=ref_id, tracking_status=bool(tracked), keypoints=kp3, descriptors=q["descriptors"][:n], camera=cam,
                                          matched_keypoints=first["matched_keypoints"], matched_keypoint_ids=first["matched_keypoint_ids"],
                                          matched_point3D_ids=first["matched_point3D_ids"])
                ret = sm.refine_pose_by_matching(q_frame)
            assert np.array_equal(handed["pts2d"], ret["matched_keypoints"] + 0.5) and np.array_equal(handed["pts3d"], ret["matched_xyzs"])
            votes = RR.find_reference_frames(map_, ret["matched_point3D_ids"][inlier_pattern(len(handed["pts2d"]))], keys, with_counts=True)[:RR.COVIS + 1]
            assert len({c for _, c in votes}) == len(votes), f"case {i}: the vote has a tie {votes}: pick another case"
            out[f"case{i}_query"] = np.array([b, ref_id, tracked])
            out[f"case{i}_kpt_ids"] = np.asarray(ret["matched_keypoint_ids"]).astype(np.int64)
            out[f"case{i}_point_ids"] = np.asarray(ret["matched_point3D_ids"]).astype(np.int64)
            out[f"case{i}_sids"] = np.asarray(ret["matched_sids"]).astype(np.int32)
            out[f"case{i}_best"] = np.asarray(ret["refinement_reference_frame_ids"]).astype(np.int64)
            out[f"case{i}_used_init"] = int(bool(tracked) and ref_id in list(sm.covisible_graph[ref_id]))
            print(f"  case {i}: query {b} ref {ref_id} tracked {tracked}: {len(ret['matched_keypoint_ids'])} rows, vote {out[f'case{i}_best'].tolist()}")
    finally:
        torch.Tensor.cuda = orig_cuda
    G.save("refine_matching_pinned", **out)


if __name__ == "__main__":
    main()
