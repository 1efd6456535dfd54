"""CPU: the numpy restatement tests/retrieval_ref.py against what the reference's pose_estimator.py produced on covisible_scene
(tests/golden/retrieval_pinned.npz, written by tests/tools/gen_retrieval_pinned.py), and DatabaseStore's host tables.  The public
covisibility_pairs runs on the device: tests/test_gpu_retrieval.py compares it with the restatement checked here."""
import numpy as np
import pytest

from tests import refine_ref as RR
from tests import retrieval_ref as TR

MIN_SIM, COVIS_K = 0.7, 3
# tests/tools/gen_retrieval_pinned.py's ITERATIVE
ITERATIVE = (("accept0", 0, (60,), 50, False, 0), ("accept_later", 0, (20, 30), 25, False, 3), ("best_taken", 1, (12, 30, 11), 50, False, 0),
             ("with_opt", 0, (20, 30, 40), 25, True, 3), ("failed", 1, (5, 9, 3), 50, False, 0))


@pytest.fixture(scope="module")
def scene():
    m, qs, _ = RR.covisible_scene()
    return m, [{k: (v[:q["count"]] if isinstance(v, np.ndarray) else v) for k, v in q.items() if k != "padded"} for q in qs]


@pytest.fixture(scope="module")
def pinned(golden):
    g = golden("retrieval_pinned")
    assert int(g["seed"]) == 7 and float(g["min_sim"]) == MIN_SIM and int(g["covis_k"]) == COVIS_K
    return g


def scripted_inliers(n, want):
    inl = np.arange(n) % 3 != 0
    inl[np.nonzero(inl)[0][want:]] = False
    return inl


def scripted_solver(answers, refine_answer=None):
    """The generator's solver: the reference calls it for the slots with 8 rows or more, in order; the k-th such call is
    answered with answers[k] inliers.  A slot the reference never reached is answered with every third row out."""
    left = list(answers)

    def solve(kpts, xyzs, tag):
        n = len(kpts)
        if tag[0] == "slot" and n < 8:
            return {"success": False}
        want = refine_answer if tag[0] == "refine" else (left.pop(0) if left else n)
        inl = scripted_inliers(n, n if want is None else want)
        return {"success": True, "inliers": inl, "num_inliers": int(inl.sum()), "qvec": np.array([1.0, 0, 0, 0]), "tvec": np.full(3, float(tag[-1]) if len(tag) > 1 else -1.0)}
    return solve


def test_covisibility_lists_equal_the_reference(scene, pinned):
    m, _ = scene
    seen = 0
    for fid in RR.frame_ids(m):
        if fid == 102:
            continue
        for k in (COVIS_K, 50):
            want = TR.get_covisibility_frames(m, fid, k + 1, with_counts=True)
            assert len({c for _, c in want}) == len(want), "the compared list has a tie"
            assert TR.get_covisibility_frames(m, fid, k) == pinned[f"covis{k}_{fid}"].tolist(), (fid, k)
            seen += 1
    assert seen == 14


def test_frame_102_ties_in_the_canonical_order(scene):
    m, _ = scene
    assert TR.get_covisibility_frames(m, 102, 5, with_counts=True) == [(100, 40), (101, 40)]
    assert TR.get_covisibility_frames(m, 102, 1) == [100]
    # all 40 rows of frame 102 carry a point it shares with both neighbours: self included, a three-way tie by frame index
    assert TR.get_covisibility_frames(m, 102, 5, include_self=True, with_counts=True) == [(100, 40), (101, 40), (102, 40)]


def test_hloc_stacks_equal_the_reference(scene, pinned):
    m, qs = scene
    mnn = RR.mnn_matcher(MIN_SIM)
    for b in range(5):
        r = TR.pose_estimator_hloc(qs[b], m, list(TR.SCENE_RETRIEVAL[b]), lambda d, tag: mnn(d), scripted_solver(()))
        if b == 4:      # an empty list: IndexError in the reference, defined here
            assert not r["success"] and r["qvec"] is None and r["num_inliers"] == 0 and r["reference_frame_id"] is None
            continue
        assert np.array_equal(r["matched_keypoint_ids"], pinned[f"hloc{b}_kpt_ids"]) and np.array_equal(r["matched_point3D_ids"], pinned[f"hloc{b}_point_ids"]), b
        assert r["num_inliers"] == int(pinned[f"hloc{b}_num_inliers"]) and r["order"] == -1 and r["reference_frame_id"] == TR.SCENE_RETRIEVAL[b][0]
    assert len(pinned["hloc0_kpt_ids"]) == 150 and len(pinned["hloc3_kpt_ids"]) == 0      # obs_th 3 leaves rows, and empties query 3


@pytest.mark.parametrize("case", ITERATIVE, ids=[c[0] for c in ITERATIVE])
def test_iterative_equals_the_reference(scene, pinned, case):
    name, b, answers, inlier_th, opt, obs_th = case
    m, qs = scene
    mnn = RR.mnn_matcher(MIN_SIM)
    n_slot_calls = int(pinned[f"it_{name}_n_calls"]) - int(opt)
    r = TR.pose_estimator_iterative(qs[b], m, list(TR.SCENE_RETRIEVAL[b]), lambda d, tag: mnn(d), scripted_solver(answers[:n_slot_calls], answers[-1] if opt else None),
                                    inlier_th=inlier_th, do_covisibility_opt=opt, covisibility_frame=COVIS_K, obs_th=obs_th)
    called = [j for j, p in enumerate(r["per_slot"]) if len(p["matched_keypoint_ids"]) >= 8][:n_slot_calls]
    assert len(called) == n_slot_calls
    for i, j in enumerate(called):      # what the reference handed its solver, call by call, up to its early stop
        assert np.array_equal(r["per_slot"][j]["matched_keypoint_ids"], pinned[f"it_{name}_call{i}_kpt_ids"]), (name, i)
        assert np.array_equal(r["per_slot"][j]["matched_point3D_ids"], pinned[f"it_{name}_call{i}_point_ids"]), (name, i)
    if name == "failed":
        assert (r["kept"], r["status"]) == (-1, 0) and r["num_inliers"] == -1 and r["qvec"] is None
        return
    assert r["order"] == int(pinned[f"it_{name}_order"]) and r["reference_frame_id"] == int(pinned[f"it_{name}_dbname"]), name
    assert r["status"] == (2 if name == "best_taken" else 1)
    if name == "best_taken":      # the reference reports the LAST slot's 11 inliers (:588-590); here the best slot's
        assert int(pinned[f"it_{name}_num_inliers"]) == 11 and r["num_inliers"] == 30 and r["kept"] == r["best"] == 1
    elif not opt:
        assert r["num_inliers"] == int(pinned[f"it_{name}_num_inliers"])
    if opt:
        i = n_slot_calls
        x = r["refinement"]
        assert np.array_equal(x["matched_keypoint_ids"], pinned[f"it_{name}_call{i}_kpt_ids"]) and np.array_equal(x["matched_point3D_ids"], pinned[f"it_{name}_call{i}_point_ids"])
        assert r["num_inliers"] == 40 and float(pinned[f"it_{name}_call{i}_max_error"]) == 9.0


def test_refinement_stack_equals_the_reference(scene, pinned):
    m, qs = scene
    mnn = RR.mnn_matcher(MIN_SIM)
    x = TR.pose_refinement(qs[1], m, 105, lambda d, tag: mnn(d), scripted_solver((), None), covisibility_frame=COVIS_K, obs_th=2, qvec=None, tvec=None)
    assert x["covisible_frame_ids"] == pinned["refine_db_ids"].tolist()
    assert np.array_equal(x["matched_keypoint_ids"], pinned["refine_kpt_ids"]) and np.array_equal(x["matched_point3D_ids"], pinned["refine_point_ids"])


def test_select_branches():
    s = lambda succ, inl, cnt, th=50, mb=10: TR.select(succ, inl, cnt, th, mb)
    assert s([1, 1], [60, 99], [20, 20]) == (0, 1, 0)
    assert s([1, 1, 1, 1], [30, 45, 40, 50], [9, 9, 9, 9]) == (3, 1, 3)
    assert s([1, 1], [99, 50], [7, 8]) == (1, 1, 1)
    assert s([0, 0], [99, 99], [20, 20]) == (-1, 0, -1)
    assert s([1, 1], [10, 4], [20, 20]) == (0, 2, 0) and s([1, 1], [9, 4], [20, 20]) == (-1, 0, 0)
    assert s([1, 1, 1], [20, 30, 30], [20, 20, 20]) == (1, 2, 1)
    assert s([1, 1], [0, 0], [0, 0]) == (-1, 0, -1)


def test_database_store_tables(scene):
    from pram_amd.localization.retrieval import DatabaseStore
    m, _ = scene
    store = DatabaseStore(m["frames"])
    pf = RR.point_frames(m)
    assert store.valid_off[0] == 0 and store.valid_off[-1] == store.n_valid == len(store.valid_rows) and store.valid_off.dtype == np.int32
    for f, fr in enumerate(m["frames"]):
        assert np.array_equal(store.valid(f) - store.frame_off[f], TR.valid_rows(fr, pf)), f
    assert store.frame_off[2] - store.frame_off[1] - len(store.valid(1)) == RR.LOST_ROWS
    ids = np.array(sorted(pf) + [-1, 5, 10 ** 12], dtype=np.int64)
    assert store.observations(ids).tolist() == [len(pf[i]) for i in sorted(pf)] + [0, 0, 0]
    assert sorted(np.bincount(store.observations(store.pt_ids)).tolist()[1:]) == sorted([154, 97, 211, 30])
    assert len(store.lm_frame) == 0 and len(store.covis_frames) == 0 and not store.is_vrf.any() and store.poses is None
    # frames without keypoint_segs, a point table that leaves ids out: their rows are not valid, their observations 0
    frames = [{k: v for k, v in fr.items() if k != "keypoint_segs"} for fr in m["frames"][:3]]
    known = {p: v for p, v in pf.items() if p % 3}
    lean = DatabaseStore(frames, point3D_frame_ids=known, poses={100 + f: (np.array([1.0, 0, 0, 0]), np.full(3, float(f))) for f in range(3)})
    for f, fr in enumerate(frames):
        want = [i for i, p in enumerate(fr["point3D_ids"].tolist()) if p in known]
        assert (lean.valid(f) - lean.frame_off[f]).tolist() == want and 0 < len(want) < len(fr["point3D_ids"]), f
    dropped = [p for p in pf if p % 3 == 0][:5]
    assert lean.observations(dropped).tolist() == [0] * 5 and lean.poses[1][2].tolist() == [2.0, 2.0, 2.0]
    # observations count duplicates and drop frames the store does not hold
    assert lean.observations([next(iter(known))])[0] == sum(g in (100, 101, 102) for g in known[next(iter(known))])
    with pytest.raises(ValueError):
        lean.indices([100, 999])
    with pytest.raises(ValueError):
        DatabaseStore(frames, poses={100: (np.zeros(4), np.zeros(3))})


def test_database_store_from_a_triangulated_map(scene):
    """The dict triangulate_map / map_tables return (per frame point3D_ids and xyzs, point3D_frame_ids from the tracks) plus the
    feature frames is all a DatabaseStore needs: no labels, no reference frames."""
    from pram_amd.localization.retrieval import DatabaseStore
    from pram_amd.localization.triangulation import map_tables
    m, _ = scene
    feats = [{k: f[k] for k in ("id", "keypoints", "descriptors", "width", "height")} for f in m["frames"]]
    # tracks as build_tracks gives them on the host, every one accepted: the scene's points, entries in ascending row
    frame_off = np.concatenate([[0], np.cumsum([len(f["keypoints"]) for f in feats])]).astype(np.int32)
    row_pid = np.concatenate([f["point3D_ids"] for f in m["frames"]])
    rows = np.nonzero(row_pid != -1)[0]
    pids, inv = np.unique(row_pid[rows], return_inverse=True)
    order = np.argsort(inv, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(pids)))]).astype(np.int32)
    xyz = np.concatenate([f["xyzs"] for f in m["frames"]])[rows][order][off[:-1]]
    trk_row = rows[order]
    trk_frame = np.searchsorted(frame_off, trk_row, side="right") - 1
    tracks = {"trk_off": off, "trk_row": trk_row.astype(np.int32), "trk_frame": trk_frame.astype(np.int32), "trk_kpt": (trk_row - frame_off[trk_frame]).astype(np.int32)}
    tri = {"accept": np.ones(len(pids), dtype=bool), "xyz": xyz, "error": np.zeros(len(pids)), "entry_keep": np.ones(len(rows), dtype=bool)}
    mapped = map_tables(np.array(RR.frame_ids(m)), frame_off, tracks, tri)
    store = DatabaseStore.from_triangulation(feats, mapped)
    assert store.n_valid == len(rows) and np.array_equal(store.valid_rows, rows) and len(store.pt_ids) == len(pids)
    direct = DatabaseStore(m["frames"])
    # the ids are map_tables' own (1-based, in track order); the structure is the scene's
    assert np.array_equal(np.sort(np.diff(store.pt_off)), np.sort(np.diff(direct.pt_off))) and np.array_equal(store.valid_off, direct.valid_off)
    assert np.array_equal(store.xyzs[rows], direct.xyzs[rows])
    with pytest.raises(ValueError):
        DatabaseStore.from_triangulation(feats[:-1], mapped)


def test_covisibility_pairs_restatement(scene, pinned):
    """The restatement's pairs list: the pinned lists for every tie-free frame, the canonical order for 102, and — self included —
    the covisibility graph ReferenceStore tabulates on the host."""
    from pram_amd.localization.candidates import ReferenceStore
    m, _ = scene
    pairs = TR.covisibility_pairs(m, COVIS_K)
    for fid in RR.frame_ids(m):
        got = [g for f, g in pairs if f == fid]
        assert got == ([100, 101] if fid == 102 else pinned[f"covis{COVIS_K}_{fid}"].tolist()), fid
    assert all(f != g for f, g in pairs) and [f for f, _ in pairs] == sorted(f for f, _ in pairs)
    store = ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, covisibility_frame=RR.COVIS)
    for f, fid in enumerate(store.frame_ids):
        if store.is_vrf[f]:
            want = TR.get_covisibility_frames(m, fid, RR.COVIS, include_self=True)
            assert [store.frame_ids[g] for g in store.covisible(f)] == want, fid
