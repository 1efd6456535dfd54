"""Writes tests/golden/retrieval_pinned.npz: what the REFERENCE's get_covisibility_frames, pose_estimator_hloc,
pose_estimator_iterative and pose_refinement (localization/pose_estimator.py) produce on tests/refine_ref.py::covisible_scene.

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are); never runs in
the test suite.  db_images, points3D and a dict standing in for the feature file are built from the scene, the network is replaced
by refine_ref's numpy mutual-nearest-neighbour matcher and pycolmap's solver by a recorder that keeps what it is handed and gives
a scripted answer: ``inliers[i] = i % 3 != 0`` cut so that num_inliers is what the script says for that call.  The fixture holds
results only: the covisibility lists, the keypoint ids / point ids of the rows every solver call was handed, and the frame the
iterative form chose.  The scene regenerates from the seed.

    python tests/tools/gen_retrieval_pinned.py
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
from tests import retrieval_ref as TR  # noqa: E402

SEED, MIN_SIM, COVIS_K = 7, 0.7, 3
# pose_estimator_iterative: (query, scripted num_inliers per solver call in call order, inlier_th, do_covisibility_opt, obs_th)
ITERATIVE = (("accept0", 0, (60,), 50, False, 0), ("accept_later", 0, (20, 30), 25, False, 3), ("best_taken", 1, (12, 30, 11), 50, False, 0),
             ("with_opt", 0, (20, 30, 40), 25, True, 3), ("failed", 1, (5, 9, 3), 50, False, 0))


def scripted_inliers(n: int, want: int) -> np.ndarray:
    """every row whose index is no multiple of 3, cut to ``want`` inliers"""
    inl = np.arange(n) % 3 != 0
    inl[np.nonzero(inl)[0][want:]] = False
    return inl


def main():
    G.import_reference()
    G._stub_missing_modules()
    import localization.pose_estimator as ref
    map_, queries, _ = RR.covisible_scene(SEED)
    ids = RR.frame_ids(map_)
    pf = RR.point_frames(map_)
    xyz_of = {}
    for f in map_["frames"]:
        for pid, x in zip(f["point3D_ids"].tolist(), f["xyzs"]):
            xyz_of.setdefault(pid, x)
    points3D = {pid: SimpleNamespace(xyz=xyz_of[pid], image_ids=np.array(fr)) for pid, fr in pf.items()}
    db_images = {fid: SimpleNamespace(name=f"db{fid}", point3D_ids=f["point3D_ids"], qvec=np.array([1.0, 0, 0, 0]), tvec=np.zeros(3))
                 for fid, f in zip(ids, map_["frames"])}
    feature_file = {f"db{fid}": {"keypoints": f["keypoints"][:, :2], "scores": f["keypoints"][:, 2], "descriptors": f["descriptors"].T,
                                 "image_size": np.array([f["width"], f["height"]])} for fid, f in zip(ids, map_["frames"])}
    point_of, kpt_of = {np.asarray(x, dtype=np.float64).tobytes(): pid for pid, x in xyz_of.items()}, []
    assert len(point_of) == len(xyz_of)
    for b, q in enumerate(queries):
        n = q["count"]
        feature_file[f"q{b}"] = {"keypoints": q["keypoints"][:n], "scores": q["scores"][:n], "descriptors": q["descriptors"][:n].T,
                                 "image_size": np.array([q["width"], q["height"]])}
        kpt_of.append({tuple(k): i for i, k in enumerate(q["keypoints"][:n].tolist())})
        assert len(kpt_of[b]) == n, "two keypoints of a query share a pixel: the recorder cannot tell them apart"
    mnn = RR.mnn_matcher(MIN_SIM)
    matcher = lambda d: {"matches0": torch.from_numpy(mnn({"descriptors0": d["descriptors0"][0].numpy(), "descriptors1": d["descriptors1"][0].numpy()}))[None]}
    calls, script = [], []

    def solver(pts2d, pts3d, camera, estimation_options=None, refinement_options=None):
        pts2d, pts3d = np.array(pts2d), np.array(pts3d)
        calls.append((pts2d, pts3d, estimation_options["ransac"]["max_error"]))
        inl = scripted_inliers(len(pts2d), script.pop(0) if script else len(pts2d))
        return {"num_inliers": int(inl.sum()), "inliers": inl, "cam_from_world": mock.MagicMock()}
    ref.pycolmap.absolute_pose_estimation = solver
    qinfo = ("SIMPLE_PINHOLE", RR.CAMERA[0], RR.CAMERA[1], [500.0, 320.0, 240.0])

    def rows(b, call):
        pts2d, pts3d, _ = call
        return (np.array([kpt_of[b][tuple(k)] for k in (pts2d - 0.5).astype(np.float32).tolist()], dtype=np.int64),
                np.array([point_of[x.tobytes()] for x in pts3d], dtype=np.int64))

    def query_data(b):
        ff = feature_file[f"q{b}"]
        return {"keypoints": ff["keypoints"], "scores": ff["scores"], "descriptors": ff["descriptors"].T, "image_size": ff["image_size"]}

    out = {"seed": SEED, "min_sim": MIN_SIM, "covis_k": COVIS_K}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self        # harness shim: the generator runs without a GPU
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            # ---- get_covisibility_frames: every frame but 102, whose two neighbours tie
            for fid in ids:
                if fid == 102:
                    continue
                for k in (COVIS_K, 50):
                    lst = [int(x) for x in ref.get_covisibility_frames(fid, db_images, points3D, covisibility_frame=k)]
                    cnt = [c for _, c in TR.get_covisibility_frames(map_, fid, k + 1, with_counts=True)]
                    assert len(set(cnt)) == len(cnt), (fid, cnt)
                    out[f"covis{k}_{fid}"] = np.array(lst, dtype=np.int64)
            # ---- pose_estimator_hloc, queries 0 .. 3 (an empty list is an IndexError in the reference)
            for b in range(4):
                calls.clear()
                r = ref.pose_estimator_hloc(f"q{b}", qinfo, list(TR.SCENE_RETRIEVAL[b]), db_images, points3D, feature_file, 12, "", matcher)
                assert len(calls) <= 1
                k, p = rows(b, calls[0]) if calls else (np.zeros(0, np.int64), np.zeros(0, np.int64))
                out[f"hloc{b}_kpt_ids"], out[f"hloc{b}_point_ids"], out[f"hloc{b}_num_inliers"] = k, p, int(r["num_inliers"])
            # ---- pose_estimator_iterative on scripted answers, one per branch
            for name, b, answers, inlier_th, opt, obs_th in ITERATIVE:
                calls.clear()
                script[:] = list(answers)
                r = None
                try:      # "failed": :601 raises TypeError, only the solver's inputs up to there are pinned
                    r = ref.pose_estimator_iterative(f"q{b}", qinfo, list(TR.SCENE_RETRIEVAL[b]), db_images, points3D, feature_file, 12, "", matcher,
                                                     inlier_th=inlier_th, do_covisibility_opt=False, covisibility_frame=COVIS_K, obs_th=obs_th)
                except TypeError:
                    assert name == "failed"
                if opt:      # :515 and :567 call pose_refinement without query_data (a TypeError): it is called here, as they meant to
                    ref.pose_refinement(query_data=query_data(b), query_cam=None, feature_file=feature_file, db_frame_id=int(r["dbname"][2:]),
                                        db_images=db_images, points3D=points3D, matcher=matcher, covisibility_frame=COVIS_K, obs_th=obs_th, opt_th=9)
                out[f"it_{name}_n_calls"] = len(calls)
                for i, c in enumerate(calls):
                    out[f"it_{name}_call{i}_kpt_ids"], out[f"it_{name}_call{i}_point_ids"] = rows(b, c)
                    out[f"it_{name}_call{i}_max_error"] = c[2]
                if r is not None:
                    out[f"it_{name}_order"], out[f"it_{name}_num_inliers"] = int(r["order"]), int(r["num_inliers"])
                    out[f"it_{name}_dbname"] = int(r["dbname"][2:])
            # ---- pose_refinement on its own: the stack of the frames covisible with 105, query 1
            calls.clear()
            r = ref.pose_refinement(query_data=query_data(1), query_cam=None, feature_file=feature_file, db_frame_id=105, db_images=db_images,
                                    points3D=points3D, matcher=matcher, covisibility_frame=COVIS_K, obs_th=2, opt_th=12)
            out["refine_kpt_ids"], out["refine_point_ids"] = rows(1, calls[0])
            out["refine_db_ids"] = np.array([int(x) for x in r["db_ids"]], dtype=np.int64)
    finally:
        torch.Tensor.cuda = orig_cuda
    for k in sorted(out):
        if k.startswith("it_") and k.endswith(("order", "n_calls", "dbname", "num_inliers")):
            print(f"  {k} = {out[k]}")
        elif k.endswith("kpt_ids"):
            print(f"  {k}: {len(out[k])} rows")
    G.save("retrieval_pinned", **out)


if __name__ == "__main__":
    main()
