"""CPU: the store's point-to-frames table and covisibility graph (pram_amd.localization.candidates.ReferenceStore) against the
numpy restatement tests/refine_ref.py, and the restatement against what the reference itself produced
(tests/golden/refine_matching_pinned.npz, written by tests/tools/gen_refine_pinned.py)."""
import numpy as np
import pytest

from tests import refine_ref as RR

from pram_amd.localization.candidates import ReferenceStore
from pram_amd.localization import refine as _refine_module  # noqa: F401  (the public call exists)


def _store(map_, **kw):
    return ReferenceStore(map_["frames"], map_["seg_ref_frame_ids"], map_.get("start_sid", 0), point3D_frame_ids=map_.get("point3D_frame_ids"), **kw)


def _check_store(map_, n_frame):
    store = _store(map_, covisibility_frame=n_frame)
    ids = RR.frame_ids(map_)
    index = {fid: i for i, fid in enumerate(ids)}
    F = len(ids)
    # the point table
    pf = RR.point_frames(map_)
    assert store.pt_ids.dtype == np.int64 and np.array_equal(store.pt_ids, np.array(sorted(pf), dtype=np.int64)) and -1 not in store.pt_ids
    assert store.pt_off.shape == (len(pf) + 1,) and store.pt_off[0] == 0 and store.pt_off[-1] == len(store.pt_frames) and store.pt_frames.dtype == np.int32
    for i, pid in enumerate(store.pt_ids.tolist()):
        got = store.pt_frames[store.pt_off[i]:store.pt_off[i + 1]].tolist()
        assert got == [index[x] for x in pf[pid]], pid
    # vrf frames and the graph
    vrf = RR.vrf_frame_ids(map_)
    assert store.is_vrf.shape == (F,) and [ids[i] for i in np.nonzero(store.is_vrf)[0]] == vrf
    graph = RR.covisibility_graph(map_, n_frame, with_counts=True)
    assert store.covis_off.shape == (F + 1,) and store.covis_off[-1] == len(store.covis_frames) == len(store.covis_count)
    for i, fid in enumerate(ids):
        got = store.covisible(i)
        cnt = store.covis_count[store.covis_off[i]:store.covis_off[i + 1]]
        want = graph.get(fid, [])
        assert [ids[g] for g in got] == [g for g, _ in want] and cnt.tolist() == [c for _, c in want], (fid, got, want)
        assert len(got) <= n_frame
    return store, graph


def test_store_tables_on_the_scene():
    map_, queries, _ = RR.covisible_scene()
    rows = [f["keypoints"].shape[0] for f in map_["frames"]]
    assert len(rows) == 8 and min(rows) < 64 and max(rows) > 128 and 40 <= min(rows) and max(rows) <= 190
    assert [q["count"] for q in queries] == [150, 100, 64, 10, 0] and all(q["padded"]["keypoints"].shape[0] == 192 for q in queries)
    store, graph = _check_store(map_, RR.COVIS)
    assert store.covisible(2).size == 0 and not store.is_vrf[2]      # nobody's reference frame: no list
    assert all(len(v) == RR.COVIS for v in graph.values())           # every list is cut
    assert all(v[0][0] == fid for fid, v in graph.items())           # a frame shares most points with itself
    _check_store(map_, 20)                                           # longer than any list: nothing is cut
    # neighbours share many points, frames two apart fewer
    g = RR.covisibility_graph(map_, 20, with_counts=True)
    c = dict(g[103])
    assert c[104] > c[105] > 0


def _hand_map():
    fr = lambda fid, ids: {"id": fid, "keypoints": np.zeros((len(ids), 3), np.float32), "descriptors": np.zeros((len(ids), 128), np.float32),
                           "xyzs": np.zeros((len(ids), 3)), "point3D_ids": np.array(ids, dtype=np.int64),
                           "keypoint_segs": np.zeros(len(ids), np.int32), "width": 640, "height": 480}
    return {"frames": [fr(10, [1, 2, -1, 7, 5]), fr(11, [1, 3, 1]), fr(12, [2, 3]), fr(13, [3, 5])],
            "seg_ref_frame_ids": {0: [10, 11], 1: [12]}, "start_sid": 0,
            # duplicate frame ids (counted), a frame outside the store (99, dropped), point id -1 (ignored), no entry for point 7
            "point3D_frame_ids": {1: [10, 11, 11], 2: [10, 12, 99], 3: [11, 12, 13], -1: [10], 5: [13, 10]}}


def test_store_tables_hand_written():
    m = _hand_map()
    store, _ = _check_store(m, 3)
    assert store.pt_ids.tolist() == [1, 2, 3, 5] and store.is_vrf.tolist() == [1, 1, 1, 0]
    assert store.pt_frames[store.pt_off[0]:store.pt_off[1]].tolist() == [0, 1, 1]      # the duplicate is kept
    assert store.pt_frames[store.pt_off[1]:store.pt_off[2]].tolist() == [0, 2]         # frame 99 is dropped
    # frame 10: rows 1 -> {10, 11, 11}, 2 -> {10, 12}, -1 and 7 skipped, 5 -> {13, 10}: 10: 3, 11: 2, 12: 1, 13: 1; the tie at the
    # cut goes to the smaller index
    assert store.covisible(0).tolist() == [0, 1, 2] and store.covis_count[:3].tolist() == [3, 2, 1]
    # frame 11: row multiplicity (point 1 twice): 11: 5, 10: 2, then 12 and 13 tie with 1
    assert store.covisible(1).tolist() == [1, 0, 2]
    # frame 12: 12: 2, then 10, 11, 13 tie with 1: ascending index
    assert store.covisible(2).tolist() == [2, 0, 1] and store.covisible(3).size == 0
    big, _ = _check_store(m, 10)      # covisibility_frame larger than the number of frames
    assert big.covisible(2).tolist() == [2, 0, 1, 3] and big.covisible(0).tolist() == [0, 1, 2, 3]
    # derived from the rows instead: one entry per row, ascending frame index
    m2 = dict(m, point3D_frame_ids=None)
    derived, _ = _check_store(m2, 10)
    assert derived.pt_ids.tolist() == [1, 2, 3, 5, 7]
    assert derived.pt_frames[derived.pt_off[0]:derived.pt_off[1]].tolist() == [0, 1, 1]
    with pytest.raises(ValueError):
        _store(m, covisibility_frame=0)


def test_find_reference_frames_restatement():
    m = _hand_map()
    cand = RR.vrf_frame_ids(m)
    # multiplicity of the matched ids and of the lists, the non-vrf frame 13 ignored, the unknown id 7 ignored, the tie by index
    got = RR.find_reference_frames(m, [1, 1, 3, 7, 2], cand, with_counts=True)
    assert got == [(11, 5), (10, 3), (12, 2)]
    assert RR.find_reference_frames(m, [3, 2], cand) == [12, 10, 11]
    assert RR.find_reference_frames(m, [], cand) == []


def test_old_attributes_unchanged():
    """A store built without the new arguments: the attributes the candidate stage reads are what they were."""
    map_, _, _ = RR.covisible_scene()
    a = ReferenceStore(map_["frames"], map_["seg_ref_frame_ids"], 0)
    b = ReferenceStore(map_["frames"], map_["seg_ref_frame_ids"], 0, point3D_frame_ids=RR.point_frames(map_), covisibility_frame=3)
    for name in ("frame_off", "keypoints", "scores", "descriptors", "xyzs", "point3D_ids", "keypoint_segs", "frame_size", "frame_norm", "sel_rows",
                 "hist_label", "hist_cnt", "hist_off", "lm_frame", "lm_sel_off", "lm_sel_len"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.frame_ids == b.frame_ids and a.start_sid == b.start_sid == 0 and a.covisibility_frame == 20
    assert np.array_equal(a.pt_ids, b.pt_ids) and np.array_equal(a.pt_frames, b.pt_frames)      # the dict given = the dict derived


def test_restatement_reproduces_the_reference(golden):
    """Pinned by execution: the reference's build_covisibility_graph, find_reference_frames and refine_pose_by_matching were run on
    covisible_scene with the numpy mutual-nearest-neighbour matcher in place of the network and a recorder in place of pycolmap's
    solver; the restatement with the same matcher hands the solver the same rows and finds the same frames."""
    g = golden("refine_matching_pinned")
    map_, queries, _ = RR.covisible_scene(int(g["seed"]))
    n_frame = int(g["covisibility_frame"])
    graph = RR.covisibility_graph(map_, n_frame)
    assert sorted(graph) == g["graph_keys"].tolist()
    for fid, lst in zip(g["graph_keys"].tolist(), g["graph_lists"]):
        assert graph[fid] == lst[lst >= 0].tolist(), fid
    matcher = RR.mnn_matcher(float(g["min_sim"]))
    n_cases = 0
    for i in range(int(g["n_cases"])):
        b, ref_id, tracked = (int(v) for v in g[f"case{i}_query"])
        q = {k: (v[:queries[b]["count"]] if isinstance(v, np.ndarray) else v) for k, v in queries[b].items() if k != "padded"}
        first = RR.match_frame(q, map_["frames"][RR.frame_ids(map_).index(ref_id)], matcher)
        located = dict(first, reference_frame_id=ref_id, tracking_status=bool(tracked))
        out = RR.refine_by_matching(q, map_, located, lambda d, j: matcher(d), lambda k, x: {"success": True, "inliers": np.arange(len(k)) % 3 != 0},
                                    covisibility_frame=n_frame, graph=graph)
        assert np.array_equal(out["matched_keypoint_ids"], g[f"case{i}_kpt_ids"]) and np.array_equal(out["matched_point3D_ids"], g[f"case{i}_point_ids"])
        assert np.array_equal(out["matched_sids"], g[f"case{i}_sids"])
        assert out["refinement_reference_frame_ids"] == g[f"case{i}_best"].tolist() and out["reference_frame_id"] == int(g[f"case{i}_best"][0])
        assert out["used_init"] == bool(g[f"case{i}_used_init"])
        n_cases += 1
    assert n_cases >= 4


def test_enable_mask_forms():
    """The ``enable`` argument of the refinements: a list, numpy bool, a tensor, None, and a wrong length."""
    import torch
    from pram_amd.localization.refine import enable_mask
    want = [1, 0, 1, 1]
    for form in (want, [True, False, True, True], np.array(want, dtype=bool), np.array(want, dtype=np.int64), np.array([[2.0, 0.0], [1.0, -1.0]]),
                 torch.tensor(want), torch.tensor(want, dtype=torch.bool)):
        on = enable_mask(form, 4, bool)
        assert on.dtype == bool and on.tolist() == [bool(x) for x in want]
    on = enable_mask(np.array(want, dtype=bool), 4)
    assert on.dtype == np.int32 and on.tolist() == want and on.flags["C_CONTIGUOUS"]
    assert enable_mask(None, 4) is None and enable_mask(None, 0) is None and enable_mask([], 0).shape == (0,)
    for bad in (want[:3], want + [1], [], torch.tensor(want[:2])):
        with pytest.raises(ValueError, match="one entry per query"):
            enable_mask(bad, 4)
