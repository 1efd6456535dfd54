"""CPU: the numpy restatement of the reference's tracker (tests/track_ref.py) against the fixture pinned by running the reference
(tests/golden/track_pinned.npz, tests/tools/gen_track_pinned.py), the state machine on sequence_scene with numpy stand-ins for the
matcher and the solver, and the host side of pram_amd.localization.tracker that needs no GPU."""
import numpy as np
import pytest

from tests import pose_ref as PR
from tests import refine_ref as RR
from tests import track_ref as TR

THRESHOLD = 4.0


def test_restatement_reproduces_the_reference(golden):
    """track_last_frame up to the solver and update_point3ds, exactly what the reference's own code produced: matches of -1,
    matches onto rows without a point, update lists with repeated keypoint ids (the last row wins), a pair without any match."""
    g = golden("track_pinned")
    cases = TR.pinned_cases(int(g["seed"]))
    assert len(cases) == int(g["n_cases"]) == 4
    repeats = 0
    for i, c in enumerate(cases):
        lists = TR.track_last_frame(c["curr"], c["last"], lambda d: c["matches0"])
        assert np.array_equal((lists["matched_keypoints"] + 0.5).astype(np.float32), g[f"case{i}_pts2d"].reshape(-1, 2)), i
        assert np.array_equal(lists["matched_xyzs"].view(np.uint64), g[f"case{i}_pts3d"].reshape(-1, 3).view(np.uint64)), i
        assert np.array_equal(lists["matched_keypoint_ids"], g[f"case{i}_kpt_ids"]) and np.array_equal(lists["matched_point3D_ids"], g[f"case{i}_point_ids"])
        assert np.array_equal(lists["matched_sids"], g[f"case{i}_sids"]) and np.array_equal(lists["matched_ref_keypoints"], g[f"case{i}_ref_kpts"].reshape(-1, 2))
        frame = TR.initialize_localization_variables(dict(c["curr"]), c["curr"]["seg_ids"])
        TR.update_point3ds(frame, c["update"])
        assert np.array_equal(frame["xyzs"].view(np.uint64), g[f"case{i}_after_xyzs"].view(np.uint64)), i
        assert np.array_equal(frame["seg_ids"], g[f"case{i}_after_seg_ids"]) and np.array_equal(frame["point3D_ids"], g[f"case{i}_after_point_ids"]), i
        ids = c["update"]["matched_keypoint_ids"]
        repeats += len(ids) - len(np.unique(ids))
    assert repeats >= 30 and len(g["case3_kpt_ids"]) == 0 and len(g["case0_kpt_ids"]) > 50


def test_update_point3ds_last_row_wins():
    f = TR.initialize_localization_variables({"keypoints": np.zeros((4, 2), np.float32)}, np.array([5, 6, 7, 8]))
    TR.update_point3ds(f, {"matched_keypoint_ids": np.array([2, 0, 2, 2]), "matched_xyzs": np.arange(12.0).reshape(4, 3),
                           "matched_sids": np.array([1, 2, 3, 4]), "matched_point3D_ids": np.array([10, 20, 30, 40])})
    assert f["point3D_ids"].tolist() == [20, -1, 40, -1] and f["seg_ids"].tolist() == [2, 6, 4, 8]
    assert f["xyzs"].tolist() == [[3.0, 4.0, 5.0], [0.0, 0.0, 0.0], [9.0, 10.0, 11.0], [0.0, 0.0, 0.0]]


def _cpu_callables(map_, frames_t, planted_t, min_inliers):
    """numpy stand-ins: mutual nearest neighbours for the matcher, the planted camera for the solver, the dominant landmark's
    reference frame for the candidate loop, refine_ref's refinement."""
    mm = RR.mnn_matcher()
    solve = TR.planted_solver(None, THRESHOLD)
    graph = RR.covisibility_graph(map_, RR.COVIS)
    position = {fid: i for i, fid in enumerate(RR.frame_ids(map_))}
    solver_for = lambda b: (lambda kp, xyz: solve({"matched_keypoints": kp, "matched_xyzs": xyz}, planted_t[b]))

    def refiner(b, frame, located, ret):
        if located["reference_frame_id"] not in graph:
            return None
        return RR.refine_by_matching(frame, map_, located, lambda d, j: mm(d), solver_for(b), covisibility_frame=RR.COVIS, graph=graph)

    def relocalizer(i, b, frame):
        labels = frame["seg_ids"][frame["seg_ids"] >= 0] if frame["count"] else np.zeros(0, np.int64)
        if len(labels) == 0:
            return {"success": False}
        fid = map_["seg_ref_frame_ids"][int(np.bincount(labels).argmax())][0]
        mo = RR.match_frame(frame, map_["frames"][position[fid]], mm)
        ret = solver_for(b)(mo["matched_keypoints"], mo["matched_xyzs"])
        if not ret["success"]:
            return {"success": False}
        located = dict(mo, reference_frame_id=fid, tracking_status=ret["num_inliers"] >= min_inliers)
        return dict(located, success=True, refinement=refiner(b, frame, located, ret), **{k: ret[k] for k in ("inliers", "num_inliers")})
    return (lambda b, d: mm(d)), (lambda b, lists: solve(lists, planted_t[b])), refiner, relocalizer


@pytest.mark.parametrize("refine_below,want", [(80, ["track", "track+refine", "track+refine", None]), (256, ["track+refine"] * 3 + [None]),
                                               (0, ["track", "track", "track", None])])
def test_state_machine_on_sequence_scene(refine_below, want):
    """Three steps of four streams: everything relocalises first (all lost), then stream 0 tracks, streams 1 and 2 track and — below
    refine_below — refine, then stream 2 jumps, fails to track and relocalises; stream 3 (no keypoints) stays lost throughout."""
    map_, frames, planted = TR.sequence_scene()
    min_inliers = 20
    loop = TR.TrackerLoop(TR.N_STREAMS, min_inliers=min_inliers, refine_below=refine_below)
    index = {fid: i for i, fid in enumerate(RR.frame_ids(map_))}
    sources = []
    for t in range(TR.N_FRAMES):
        qs = [TR.real(q) for q in frames[t]]
        out = loop.step(qs, list(range(TR.N_STREAMS)), *_cpu_callables(map_, frames[t], planted[t], min_inliers), seg_ids=[q["seg_ids"] for q in qs])
        sources.append([o["source"] for o in out])
        assert loop.lost == [False, False, False, True]
        st = TR.state_arrays(loop, RR.N_PAD, index)
        for s in range(3):
            n = qs[s]["count"]
            assert st["counts"][s] == n and st["ref_frame"][s] >= 0
            got, pool = st["point3D_ids"][s, :n], qs[s]["pool"]
            assert (got >= 0).sum() >= min_inliers and (got[got >= 0] == pool[got >= 0]).mean() > 0.95      # the points are the keypoints' own
            assert (st["point3D_ids"][s, n:] == -1).all() and (st["xyzs"][s, n:] == 0).all()
            bare = got < 0
            assert np.array_equal(st["seg_ids"][s, :n][bare], qs[s]["seg_ids"][bare])      # rows without a point keep the frame's own label
        assert st["counts"][3] == 0 and st["ref_frame"][3] == -1
    assert sources[0] == ["relocalize"] * 3 + [None]
    assert sources[1] == want
    assert sources[2] == [want[0], want[1], "relocalize", None]      # stream 2 was tracked, jumps, and relocalises


def test_tracker_module_without_a_gpu():
    from pram_amd import _lib
    from pram_amd._lib import PramHipError
    from pram_amd.localization import tracker as T
    for name in ("pram_track_plan", "pram_track_correspond", "pram_track_filter", "pram_track_commit"):
        assert name in _lib.exported_symbols()
    with pytest.raises(PramHipError):
        T.TrackState(2, 16, "cpu")
    with pytest.raises(ValueError):
        T.TrackState(0, 16, "cpu")
    cams = [PR.PLANTED_CAMERAS[i] for i in range(4)]
    assert T._sub_cameras(cams, [2, 0]) == [cams[2], cams[0]]
    ids, params = np.arange(4, dtype=np.int32), np.arange(32.0).reshape(4, 8)
    sub = T._sub_cameras((ids, params), [3, 1])
    assert sub[0].tolist() == [3, 1] and np.array_equal(sub[1], params[[3, 1]])
    assert "lost = not success" in T.__doc__ and "recogniser" in T.Tracker.__doc__


def test_option_groups_partition_the_tracker_keys():
    """Every keyword option of Tracker stands in exactly one group; the splitter keeps values, takes any subset, and rejects an
    unknown key the way Localizer does."""
    import inspect
    from pram_amd.localization import localizer as L
    from pram_amd.localization import tracker as T
    flat = [k for keys in T.OPTION_GROUPS.values() for k in keys]
    assert set(T.OPTION_GROUPS) == {"pose", "localize", "refine", "tracker"}
    assert sorted(flat) == sorted(T.TRACKER_KEYS) and len(set(flat)) == len(flat) == 15 and L.TRACKER_KEYS is T.TRACKER_KEYS
    sig = inspect.signature(T.Tracker.__init__).parameters
    assert {k for k, p in sig.items() if p.kind is p.KEYWORD_ONLY} - {"device"} == set(T.TRACKER_KEYS)
    # a group's keys are the keyword arguments of the stage it is handed to
    takes = lambda fn: set(inspect.signature(fn).parameters)
    from pram_amd.localization import pose, refine
    assert set(T.OPTION_GROUPS["pose"]) <= takes(pose.estimate_poses) and set(T.OPTION_GROUPS["pose"]) <= takes(refine.refine_by_projection)
    assert set(T.OPTION_GROUPS["pose"] + T.OPTION_GROUPS["localize"]) <= takes(pose.localize_candidates)
    assert set(T.OPTION_GROUPS["pose"] + T.OPTION_GROUPS["localize"] + T.OPTION_GROUPS["refine"]) <= takes(refine.localize_and_refine)
    assert not set(T.OPTION_GROUPS["tracker"]) & takes(refine.localize_and_refine)
    kw = {k: i for i, k in enumerate(T.TRACKER_KEYS)}
    g = T.split_options(kw)
    assert {k: v for d in g.values() for k, v in d.items()} == kw and all(tuple(g[n]) == T.OPTION_GROUPS[n] for n in g)
    assert T.split_options({"seed": 3, "refine_below": 9}) == {"pose": {"seed": 3}, "localize": {}, "refine": {}, "tracker": {"refine_below": 9}}
    with pytest.raises(TypeError, match=r"Localizer: unknown arguments \['n_trials', 'seg'\]"):
        T.split_options({"seg": 1, "n_trials": 2, "seed": 0}, "Localizer")
    with pytest.raises(TypeError, match="unknown arguments"):
        L.Localizer(None, None, pre_filtering_th=0.5, n_trials=3)
