"""CPU: the candidate-matching entries are declared and exported, ReferenceStore's selections are the reference's masks, and the
numpy restatement of the reference's candidate loop (tests/cand_ref.py) behaves as the cited lines say on hand-made cases."""
from pathlib import Path

import numpy as np

from tests import cand_ref as CR

ROOT = Path(__file__).resolve().parents[1]
CAND = ("pram_cand_mask_ranks", "pram_cand_plan", "pram_cand_gather", "pram_cand_correspond")


def test_cand_symbols_declared_and_exported(hip_lib):
    # the entries' declarations, types and exports and PRAM_CAND_PLAN_COLS == ops.CAND_PLAN_COLS: tests/test_abi_contract_cpu.py
    from pram_amd import _lib, ops
    assert set(CAND) <= set(_lib.exported_symbols()) and all(_lib._SIGS[n][0] is _lib.I for n in CAND)
    assert ops.CAND_PLAN_COLS == len(ops.CAND_PLAN_FIELDS) == 10


def _frame(segs, w=640, h=480, seed=0, fid=None):
    rng = np.random.default_rng(seed)
    n = len(segs)
    f = {"keypoints": rng.uniform(0, 400, (n, 3)).astype(np.float32), "descriptors": rng.standard_normal((n, 128)).astype(np.float32),
         "xyzs": rng.standard_normal((n, 3)), "point3D_ids": np.arange(n, dtype=np.int64) + 1000 * seed, "keypoint_segs": np.array(segs, dtype=np.int32),
         "width": w, "height": h}
    if fid is not None:
        f["id"] = fid
    return f


def test_store_selections_are_the_reference_masks():
    from pram_amd.localization.candidates import ReferenceStore
    frames = [_frame([3, 0, 3, 1, 0, 3, 7], seed=1, fid="a"), _frame([2], w=800, h=600, seed=2, fid="b"), _frame([], seed=3, fid="c"),
              _frame([1, 1, 0, 5, 1], seed=4, fid="d")]
    store = ReferenceStore(frames, {0: ["a"], 1: ["d", "a"], 2: ["b"], 3: ["a"], 5: ["d"], 6: []}, start_sid=4)
    assert store.n_frames == 4 and store.n_rows == 13 and store.max_frame_rows == 7
    assert store.frame_off.tolist() == [0, 7, 8, 8, 13]
    for f, fr in enumerate(frames):
        off = int(store.frame_off[f])
        assert np.array_equal(store.rows(f), off + np.arange(len(fr["keypoint_segs"])))
        for sid in (0, 1, 2, 3, 4, 5, 7, 99):      # present, absent, sid 0
            assert np.array_equal(store.rows_by_sid(f, sid), off + np.nonzero(fr["keypoint_segs"] == sid)[0]), (f, sid)
        rows = store.rows(f)
        assert np.array_equal(store.descriptors[rows], fr["descriptors"]) and np.array_equal(store.xyzs[rows], fr["xyzs"])
        assert np.array_equal(store.keypoints[rows], fr["keypoints"][:, :2]) and np.array_equal(store.scores[rows], fr["keypoints"][:, 2])
        assert np.array_equal(store.point3D_ids[rows], fr["point3D_ids"])
        # the class histogram of check_semantic_consistency
        lab = store.hist_label[store.hist_off[f]:store.hist_off[f + 1]]
        cnt = store.hist_cnt[store.hist_off[f]:store.hist_off[f + 1]]
        u, c = np.unique(fr["keypoint_segs"], return_counts=True)
        assert np.array_equal(lab, u) and np.array_equal(cnt, c)
    # per landmark: entry [0] is the reference frame; its rows of that landmark
    assert store.lm_frame.tolist() == [0, 3, 1, 0, -1, 3, -1]
    for l, f in enumerate(store.lm_frame):
        if f >= 0:
            sel = store.sel_rows[store.lm_sel_off[l]:store.lm_sel_off[l] + store.lm_sel_len[l]]
            assert np.array_equal(sel, store.rows_by_sid(int(f), l)), l
    assert store.rows_by_sid(1, 2).tolist() == [7]      # the one-keypoint frame
    # the (1, 3, width, height) quirk: centre (height / 2, width / 2)
    assert store.frame_norm[0].tolist() == [240.0, 320.0, 448.0] and store.frame_norm[1].tolist() == [300.0, 400.0, 560.0]
    assert CR.norm_constants(640, 480) == (240.0, 320.0, 448.0)
    from pram_amd.nets.utils import keypoint_norm_constants
    assert keypoint_norm_constants((1, 3, 800, 600)) == CR.norm_constants(800, 600)


def test_vote_restatement_order_and_ties():
    # 6 tokens, 4 classes; rank 0: class 2 x3, class 1 x1, background x2; rank 1 brings class 3
    segs = np.array([[0.1, 0.2, 0.9, 0.0], [0.1, 0.2, 0.9, 0.3], [0.0, 0.1, 0.8, 0.5], [0.2, 0.9, 0.1, 0.0], [0.9, 0.0, 0.1, 0.5],
                     [0.9, 0.0, 0.1, 0.6]], dtype=np.float32)
    out = CR.process_segmentations(segs, 10)
    assert [o[0] for o in out] == [2, 1, 3]
    assert out[0][1].tolist() == [0, 1, 2] and out[1][1].tolist() == [3] and out[2][1].tolist() == [1, 2, 4, 5]
    assert abs(out[0][2] - np.mean([0.9, 0.9, 0.8])) < 1e-6
    assert [o[0] for o in CR.process_segmentations(segs, 2)] == [2, 1]
    assert CR.process_segmentations(np.zeros((0, 4), np.float32), 3) == []
    # equal counts: ascending class id
    tie = np.array([[0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.float32)
    assert [o[0] for o in CR.process_segmentations(tie, 2)] == [1, 2]


def _query(cls, n_class, seed=0):
    rng = np.random.default_rng(seed)
    n = len(cls)
    seg = np.zeros((n, n_class), dtype=np.float32)
    seg[np.arange(n), cls] = 1.0
    return {"keypoints": rng.uniform(0, 400, (n, 2)).astype(np.float32), "scores": rng.uniform(0, 1, n).astype(np.float32),
            "descriptors": rng.standard_normal((n, 128)).astype(np.float32), "segmentations": seg, "seg_ids": np.array(cls, dtype=np.int32) - 1,
            "width": 640, "height": 480}


def test_restatement_branches():
    # landmarks 0 and 1 -> frame 0 with labels {0: 2 rows, 1: 4 rows, 9: 2 rows}
    m = {"frames": [_frame([1, 0, 1, 9, 1, 0, 1, 9], seed=5)], "seg_ref_frame_ids": {0: [0], 1: [0]}, "start_sid": 0}
    # 8 keypoints: 4 on class 2 (landmark 1), 2 on class 1 (landmark 0), 2 background -> share 6 / 8 and 6 / 8
    q = _query([2, 2, 0, 2, 1, 2, 0, 1], 11)
    c = CR.candidates(q, m, seg_k=2, min_kpts=2, matcher=lambda d: np.full(d["descriptors0"].shape[0], -1))
    assert [x["sid"] for x in c] == [1, 0] and [x["order"] for x in c] == [0, 1]
    assert c[0]["semantic_matching"] and c[0]["q_kpt_ids"].tolist() == [0, 1, 3, 5] and c[0]["ref_rows"].tolist() == [0, 2, 4, 6]
    # the sid > 0 rule: landmark 0 matches semantically but against the WHOLE frame
    assert c[1]["semantic_matching"] and c[1]["q_kpt_ids"].tolist() == [4, 7] and c[1]["ref_rows"].tolist() == list(range(8))
    assert c[0]["data"]["image_shape1"] == (1, 3, 640, 480) and c[0]["data"]["keypoints1"].shape == (4, 2)
    assert c[0]["matched_xyzs"].shape == (0, 3)
    # the min_kpts fallback: 2 tokens < 3 -> all keypoints, no semantic matching, whole frame
    c = CR.candidates(q, m, seg_k=2, min_kpts=3)
    assert c[0]["semantic_matching"] and not c[1]["semantic_matching"]
    assert c[1]["q_kpt_ids"].tolist() == list(range(8)) and c[1]["ref_rows"].tolist() == list(range(8))
    # the switch
    c = CR.candidates(q, m, seg_k=1, min_kpts=0, semantic_matching=False)
    assert len(c) == 1 and not c[0]["semantic_matching"] and c[0]["q_kpt_ids"].shape[0] == 8
    # overlap exactly 0.5 passes: 4 of 8 query keypoints carry a label of the frame, 4 of 8 frame rows carry label 1
    q2 = _query([2, 2, 2, 2, 0, 0, 5, 5], 11)
    assert CR.check_semantic_consistency(q2["seg_ids"], m["frames"][0], 0, 0.5)
    assert CR.candidates(q2, m, seg_k=1, min_kpts=1)[0]["semantic_matching"]
    # one keypoint less on the query side: 3 / 8 fails
    q3 = _query([2, 2, 2, 0, 0, 0, 5, 5], 11)
    assert not CR.check_semantic_consistency(q3["seg_ids"], m["frames"][0], 0, 0.5)
    assert not CR.candidates(q3, m, seg_k=1, min_kpts=1)[0]["semantic_matching"]
    # start_sid shifts the map's labels into the global numbering: class 5 = global landmark 4 = in-map landmark 1
    m3 = dict(m, start_sid=3)
    q4 = _query([5, 5, 0, 5, 4, 5, 0, 4], 11)
    c = CR.candidates(q4, m3, seg_k=2, min_kpts=2)
    assert [x["sid"] for x in c] == [4, 3] and c[0]["ref_rows"].tolist() == [0, 2, 4, 6] and c[1]["ref_rows"].tolist() == list(range(8))


def test_restatement_correspondences():
    m = {"frames": [_frame([1, 0, 1, 9, 1, 0, 1, 9], seed=5)], "seg_ref_frame_ids": {0: [0], 1: [0]}, "start_sid": 0}
    q = _query([2, 2, 0, 2, 1, 2, 0, 1], 11)
    c = CR.candidates(q, m, seg_k=1, min_kpts=2, matcher=lambda d: np.array([3, -1, 0, 1]))[0]
    fr = m["frames"][0]
    assert c["matched_keypoint_ids"].tolist() == [0, 3, 5]
    assert np.array_equal(c["matched_keypoints"], q["keypoints"][[0, 3, 5]])
    assert np.array_equal(c["matched_xyzs"], fr["xyzs"][[6, 0, 2]]) and c["matched_point3D_ids"].tolist() == fr["point3D_ids"][[6, 0, 2]].tolist()
    assert c["matched_sids"].tolist() == [1, 1, 1] and np.array_equal(c["matched_ref_keypoints"], fr["keypoints"][[6, 0, 2], :2])


def test_synthetic_map_shapes():
    m = CR.make_map(3)
    n = [f["keypoints"].shape[0] for f in m["frames"]]
    assert len(n) >= 12 and min(n) == 600 and max(n) == 1376 and {(f["width"], f["height"]) for f in m["frames"]} == set(CR.CAMERAS)
    q = CR.make_query(1, m, [(4, 100), (None, 28)], 256, 29)
    assert q["count"] == 128 and q["padded"]["descriptors"].shape == (256, 128) and (q["seg_ids"] == 4).sum() == 100
