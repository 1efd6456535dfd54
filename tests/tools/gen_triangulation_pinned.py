"""Writes tests/golden/triangulation_pinned.npz: what the REFERENCE's compute_epipolar_errors (colmap_utils/geometry.py) returns
on the verification inputs of tests/triangulation_ref.py::tri_scene — for every processed pair and every match with both indices
inside their frames, the two normalised points, the two errors and the mask geometric_verification (localization/triangulation.py)
derives from them with max_error = 4.

Needs the reference tree beside the repository (oracle/gen_golden.py names it); never runs in the test suite.  pycolmap is a
stand-in module in sys.modules: the function only calls ``essential_matrix()`` on the pose it is given, and a plain object provides
that as COLMAP defines it, E = [t / |t|]x R (EssentialMatrixFromPose), with R and t of cam1_from_cam0 composed here by numpy's
matrix products from the scene's quaternions, not by the restatement.  The thresholds are COLMAP's cam_from_img_threshold,
max_error over the mean focal length.  The fixture holds inputs and results only.

    python tests/tools/gen_triangulation_pinned.py
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import gen_golden as G  # noqa: E402
from tests import pose_ref as PR  # noqa: E402
from tests import triangulation_ref as TR  # noqa: E402


class Rigid3d:
    def __init__(self, R, t):
        self.R, self.t = R, t

    def essential_matrix(self):
        x, y, z = self.t / np.linalg.norm(self.t)
        return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]]) @ self.R


def main():
    stand_in = types.ModuleType("pycolmap")
    stand_in.Rigid3d = Rigid3d
    sys.modules["pycolmap"] = stand_in
    sys.path.insert(0, str(G.REF))
    from colmap_utils.geometry import compute_epipolar_errors
    s = TR.tri_scene()
    use = TR.unique_pairs(s["pairs"])
    R = [PR.qvec_to_rot(q / np.linalg.norm(q)) for q in s["qvec"]]
    off, x0s, x1s, errs, keeps = [0], [], [], [], []
    for i in use:
        f0, f1 = s["pairs"][i].tolist()
        m = s["matches"][i]
        n0, n1 = (int(s["frame_off"][f + 1] - s["frame_off"][f]) for f in (f0, f1))
        m = m[(m[:, 0] >= 0) & (m[:, 0] < n0) & (m[:, 1] >= 0) & (m[:, 1] < n1)]      # the reference would raise on the others
        x0, x1 = s["norm0"][s["frame_off"][f0] + m[:, 0]], s["norm0"][s["frame_off"][f1] + m[:, 1]]
        if len(m):
            R10 = R[f1] @ R[f0].T
            e0, e1 = compute_epipolar_errors(Rigid3d(R10, s["tvec"][f1] - R10 @ s["tvec"][f0]), x0, x1)
        else:
            e0 = e1 = np.zeros(0)
        th0, th1 = (4.0 / PR.f_mean(int(s["cam_model"][f]), s["cam_params"][f]) for f in (f0, f1))
        off.append(off[-1] + len(m)); x0s.append(x0); x1s.append(x1)
        errs.append(np.stack([e0, e1], 1)); keeps.append(np.logical_and(e0 <= th0, e1 <= th1))
    keep = np.concatenate(keeps)
    print(f"  {len(use)} pairs, {off[-1]} matches, {int(keep.sum())} kept")
    G.save("triangulation_pinned", pair_index=np.array(use), pairs=s["pairs"][use], match_off=np.array(off), x0=np.concatenate(x0s),
           x1=np.concatenate(x1s), errors=np.concatenate(errs), keep=keep)


if __name__ == "__main__":
    main()
