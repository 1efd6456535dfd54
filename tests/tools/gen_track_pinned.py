"""Writes tests/golden/track_pinned.npz: what the REFERENCE's Tracker.track_last_frame (localization/tracker.py) hands to the
solver, and what Frame.update_point3ds (localization/frame.py) leaves in a frame, on tests/track_ref.py::pinned_cases (frames of
sequence_scene with recorded matches0 and update lists with repeated keypoint ids).

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are); never runs in
the test suite.  The reference objects are built with __new__, torch.Tensor.cuda is the identity, the matcher is a callable that
answers with the recorded matches0, pycolmap's solver is a recorder that keeps what it is handed.  The fixture holds results only:
the rows handed to the solver with the lists the method returns, and the frame's three arrays after the update.  The cases
regenerate from the seed.

    python tests/tools/gen_track_pinned.py
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
from tests import track_ref as TR  # noqa: E402

THRESHOLD = 4.0


def ref_frame(Frame, q: dict):
    f = Frame.__new__(Frame)
    f.camera = SimpleNamespace(width=q["width"], height=q["height"])
    f.keypoints = np.concatenate([q["keypoints"], q["scores"][:, None]], 1).astype(np.float32)
    f.descriptors = q["descriptors"]
    f.initialize_localization_variables()
    f.reference_frame_id, f.matched_scene_name = q.get("reference_frame_id"), "scene"
    if "point3D_ids" in q:      # a located frame: what update_point3ds left
        f.seg_ids, f.point3D_ids, f.xyzs = q["seg_ids"].copy(), q["point3D_ids"].copy(), q["xyzs"].copy()
    return f


def main():
    G.import_reference()
    G._stub_missing_modules()
    import localization.tracker as ref_tr
    from localization.frame import Frame
    handed = {}

    def solver(pts2d, pts3d, camera, estimation_options=None, refinement_options=None):
        handed.update(pts2d=np.array(pts2d), pts3d=np.array(pts3d), max_error=estimation_options["ransac"]["max_error"])
        return {"num_inliers": len(pts2d), "inliers": np.ones(len(pts2d), dtype=bool), "cam_from_world": mock.MagicMock()}

    ref_tr.pycolmap.absolute_pose_estimation = solver
    trk = ref_tr.Tracker.__new__(ref_tr.Tracker)
    trk.config = {"localization": {"threshold": THRESHOLD}}
    cases = TR.pinned_cases(TR.SCENE_SEED)
    out = {"seed": TR.SCENE_SEED, "n_cases": len(cases)}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self        # harness shim: the generator runs without a GPU
    try:
        for i, c in enumerate(cases):
            last, curr = ref_frame(Frame, c["last"]), ref_frame(Frame, {k: v for k, v in c["curr"].items() if k not in ("seg_ids",)})
            trk.matcher = lambda data, m0=c["matches0"]: {"matches0": torch.from_numpy(m0)[None]}
            with contextlib.redirect_stdout(io.StringIO()):
                ret = trk.track_last_frame(curr_frame=curr, last_frame=last)
            assert np.array_equal(handed["pts2d"], ret["matched_keypoints"] + 0.5) and np.array_equal(handed["pts3d"], ret["matched_xyzs"])
            assert handed["max_error"] == THRESHOLD and ret["reference_frame_id"] == c["last"]["reference_frame_id"]
            n_minus = int((c["matches0"] < 0).sum())
            onto_bare = int((c["last"]["point3D_ids"][c["matches0"][c["matches0"] >= 0]] < 0).sum())
            out[f"case{i}_pts2d"], out[f"case{i}_pts3d"] = handed["pts2d"].astype(np.float32), handed["pts3d"].astype(np.float64)
            out[f"case{i}_kpt_ids"] = np.asarray(ret["matched_keypoint_ids"]).astype(np.int64)
            out[f"case{i}_point_ids"] = np.asarray(ret["matched_point3D_ids"]).astype(np.int64)
            out[f"case{i}_sids"] = np.asarray(ret["matched_sids"]).astype(np.int32)
            out[f"case{i}_ref_kpts"] = np.asarray(ret["matched_ref_keypoints"]).astype(np.float32)
            # the update, on the current frame, with the list that repeats keypoint ids
            u = c["update"]
            curr.seg_ids = c["curr"]["seg_ids"].astype(int).copy()
            curr.matched_keypoint_ids, curr.matched_xyzs = u["matched_keypoint_ids"], u["matched_xyzs"]
            curr.matched_sids, curr.matched_point3D_ids = u["matched_sids"], u["matched_point3D_ids"]
            curr.update_point3ds()
            out[f"case{i}_after_xyzs"] = np.asarray(curr.xyzs, dtype=np.float64)
            out[f"case{i}_after_seg_ids"] = np.asarray(curr.seg_ids).astype(np.int32)
            out[f"case{i}_after_point_ids"] = np.asarray(curr.point3D_ids).astype(np.int64)
            rep = len(u["matched_keypoint_ids"]) - len(np.unique(u["matched_keypoint_ids"]))
            print(f"  case {i}: stream {c['stream']} frame {c['frame']}: {len(c['matches0'])} keypoints, {n_minus} unmatched, {onto_bare} onto rows "
                  f"without a point, {len(handed['pts2d'])} rows to the solver; update list {len(u['matched_keypoint_ids'])} rows, {rep} repeats")
            if i < 3:
                assert n_minus > 0 and onto_bare > 0 and rep > 0 and len(handed["pts2d"]) > 0
    finally:
        torch.Tensor.cuda = orig_cuda
    G.save("track_pinned", **out)


if __name__ == "__main__":
    main()
