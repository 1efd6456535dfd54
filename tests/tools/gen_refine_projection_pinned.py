"""Writes tests/golden/refine_projection_pinned.npz: what the REFERENCE's refine_pose_by_projection (localization/singlemap3d.py)
produces on tests/projref_ref.py::projection_scene (refine_ref.covisible_scene with its point lists and planted localisations).

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are); never runs in
the test suite.  The reference object is built with __new__, torch.Tensor.cuda is the identity, pycolmap's solver is a recorder
that keeps what it is handed and answers with a fixed inlier pattern (every row whose index is not a multiple of 3).  Every case
gets a fresh copy of the covisibility graph, because the method appends the reference frame to the graph's own list.  The union
and the frustum mask are read from the method's local variables when it returns.  The fixture holds results only: the union's
size, the frustum mask, the keypoint ids / point ids / landmarks the solver's rows carry, and the frames of the vote.  The scene
regenerates from the seed.

    python tests/tools/gen_refine_projection_pinned.py
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
from tests import projref_ref as PJ  # noqa: E402
from tests import refine_ref as RR  # noqa: E402


def inlier_pattern(n: int) -> np.ndarray:
    return np.arange(n) % 3 != 0


def main():
    G.import_reference()
    G._stub_missing_modules()
    import localization.singlemap3d as ref_sm
    from localization.frame import Frame
    map_, queries, planted, located = PJ.projection_scene(PJ.SCENE_SEED)
    ids = RR.frame_ids(map_)
    pf = RR.point_frames(map_)
    table = PJ.point_table(map_)
    sm = ref_sm.SingleMap3D.__new__(ref_sm.SingleMap3D)
    sm.point3Ds = {int(pid): SimpleNamespace(xyz=table["xyz"][i], descriptor=table["desc"][i], seg_id=int(table["sid"][i]), frame_ids=np.array(pf[int(pid)]))
                   for i, pid in enumerate(table["ids"])}
    sm.reference_frames = {fid: SimpleNamespace(point3D_ids=f["point3D_ids"]) for fid, f in zip(ids, map_["frames"])}
    # the reference would raise KeyError on the rows without a point (id -1, singlemap3d.py:392): give them no say, as the project does
    for rf in sm.reference_frames.values():
        rf.point3D_ids = rf.point3D_ids[rf.point3D_ids != -1]
    sm.config = {"localization": {"threshold": PJ.THRESHOLD, "covisibility_frame": RR.COVIS}}
    sm.build_covisibility_graph(frame_ids=RR.vrf_frame_ids(map_), n_frame=RR.COVIS)
    built = {fid: [int(x) for x in lst] for fid, lst in sm.covisible_graph.items()}
    want = RR.covisibility_graph(map_, RR.COVIS)
    assert all(sorted(want[fid]) == sorted(built[fid]) for fid in built), "the restatement's graph differs"
    handed, seen = {}, {}

    def solver(pts2d, pts3d, camera, estimation_options=None, refinement_options=None):
        handed.update(pts2d=np.array(pts2d), pts3d=np.array(pts3d), max_error=estimation_options["ransac"]["max_error"])
        inl = inlier_pattern(len(pts2d))
        return {"num_inliers": int(inl.sum()), "inliers": inl, "cam_from_world": mock.MagicMock()}

    def profile(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "refine_pose_by_projection":
            seen.update({k: frame.f_locals[k] for k in ("all_point3D_ids", "mask", "covis_frame_ids")})
    ref_sm.pycolmap.absolute_pose_estimation = solver
    cases = [i for i, l in enumerate(located) if l is not None]
    out = {"seed": PJ.SCENE_SEED, "threshold": PJ.THRESHOLD, "covisibility_frame": RR.COVIS, "cases": np.array(cases)}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self        # harness shim: the generator runs without a GPU
    try:
        for i in cases:
            l = located[i]
            q = queries[l["query"]]
            n = q["count"]
            cam = planted[l["query"]]["cam"]
            q_frame = Frame.__new__(Frame)
            q_frame.camera = SimpleNamespace(model=SimpleNamespace(name=cam[0]), params=np.array(cam[3], dtype=np.float64), width=cam[1], height=cam[2])
            q_frame.qvec, q_frame.tvec, q_frame.reference_frame_id = np.array(l["qvec"]), np.array(l["tvec"]), l["reference_frame_id"]
            q_frame.keypoints = np.concatenate([q["keypoints"][:n], q["scores"][:n, None]], 1).astype(np.float32)
            q_frame.descriptors = q["descriptors"][:n]
            sm.covisible_graph = {fid: list(lst) for fid, lst in built.items()}      # a fresh copy: the method appends to it
            listed = l["reference_frame_id"] in sm.covisible_graph[l["reference_frame_id"]]
            sys.setprofile(profile)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    ret = sm.refine_pose_by_projection(q_frame)
            finally:
                sys.setprofile(None)
            assert np.array_equal(handed["pts2d"], ret["matched_keypoints"][:, :2] + 0.5) and np.array_equal(handed["pts3d"], ret["matched_xyzs"])
            assert handed["max_error"] == PJ.THRESHOLD and (l["reference_frame_id"] in seen["covis_frame_ids"])
            inl = inlier_pattern(len(handed["pts2d"]))
            votes = RR.find_reference_frames(map_, ret["matched_point3D_ids"][inl], built.keys(), with_counts=True)[:RR.COVIS + 1]
            assert len({c for _, c in votes}) == len(votes), f"case {i}: the vote has a tie {votes}: pick another case"
            out[f"case{i}_query"] = np.array([l["query"], l["reference_frame_id"], int(listed)])
            out[f"case{i}_n_union"] = len(seen["all_point3D_ids"])
            out[f"case{i}_mask"] = np.asarray(seen["mask"].numpy()).astype(np.uint8)
            out[f"case{i}_kpt_ids"] = np.asarray(ret["matched_keypoint_ids"]).astype(np.int64)
            out[f"case{i}_point_ids"] = np.asarray(ret["matched_point3D_ids"]).astype(np.int64)
            out[f"case{i}_sids"] = np.asarray(ret["matched_sids"]).astype(np.int32)
            out[f"case{i}_best"] = np.asarray(ret["refinement_reference_frame_ids"]).astype(np.int64)
            print(f"  case {i}: query {l['query']} ref {l['reference_frame_id']} listed {listed}: union {len(seen['all_point3D_ids'])}, "
                  f"in the frustum {int(seen['mask'].sum())}, {len(ret['matched_keypoint_ids'])} matches, vote {out[f'case{i}_best'].tolist()}")
    finally:
        torch.Tensor.cuda = orig_cuda
    assert {int(out[f"case{i}_query"][2]) for i in cases} == {0, 1}, "both kinds of reference frame are needed"
    G.save("refine_projection_pinned", **out)


if __name__ == "__main__":
    main()
