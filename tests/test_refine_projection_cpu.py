"""CPU: the store's per-point table (ReferenceStore.pt_xyz / pt_desc / pt_sid) against the numpy restatement
tests/projref_ref.py, the restatement against what the reference itself produced (tests/golden/refine_projection_pinned.npz,
written by tests/tools/gen_refine_projection_pinned.py), and the margins of the shared scene: the GPU tests excuse no decision,
so every decision of the scene has to stand clear of its bound."""
import numpy as np
import pytest

from tests import pose_ref as PR
from tests import projref_ref as PJ
from tests import refine_ref as RR

from pram_amd.localization.candidates import ReferenceStore
from pram_amd.localization.refine import refine_by_projection  # noqa: F401  (the public call exists)


def _store(map_, **kw):
    return ReferenceStore(map_["frames"], map_["seg_ref_frame_ids"], map_.get("start_sid", 0), point3D_frame_ids=map_.get("point3D_frame_ids"), **kw)


def _same_table(store, table):
    assert np.array_equal(store.pt_ids, table["ids"])
    assert store.pt_xyz.dtype == np.float64 and store.pt_xyz.shape == (len(table["ids"]), 3) and np.array_equal(store.pt_xyz, table["xyz"])
    assert store.pt_desc.dtype == np.float32 and store.pt_desc.shape == (len(table["ids"]), 128) and np.array_equal(store.pt_desc, table["desc"])
    assert store.pt_sid.dtype == np.int32 and store.pt_sid.shape == (len(table["ids"]),) and np.array_equal(store.pt_sid, table["sid"])


def test_point_table_on_the_scene():
    map_, _, _ = RR.covisible_scene()
    _same_table(_store(map_), PJ.point_table(map_))
    pmap, _, _, _ = PJ.projection_scene()
    store = _store(pmap, covisibility_frame=RR.COVIS)
    _same_table(store, PJ.point_table(pmap))
    # a shared point has one xyz and landmark in every frame: the first row's value is every row's
    at = np.searchsorted(store.pt_ids, store.point3D_ids[store.point3D_ids != -1])
    assert np.array_equal(store.pt_xyz[at], store.xyzs[store.point3D_ids != -1])
    assert np.array_equal(store.pt_sid[at], store.keypoint_segs[store.point3D_ids != -1])
    # the unlisted frame is not in its own covisible list, the others are
    index = {fid: i for i, fid in enumerate(store.frame_ids)}
    assert index[101] not in store.covisible(index[101]).tolist() and index[100] in store.covisible(index[100]).tolist()


def _hand_map():
    def fr(fid, ids, base):
        n = len(ids)
        d = np.zeros((n, 128), np.float32)
        d[:, 0] = base + np.arange(n)
        return {"id": fid, "keypoints": np.zeros((n, 3), np.float32), "descriptors": d, "xyzs": (base + np.arange(n))[:, None] * np.ones((1, 3)),
                "point3D_ids": np.array(ids, dtype=np.int64), "keypoint_segs": (base // 10 + np.arange(n)).astype(np.int32), "width": 640, "height": 480}
    # point 1 three times (two frames, twice in frame 11), -1 rows, point 9 has a list but no row
    return {"frames": [fr(10, [1, 2, -1, 7], 100), fr(11, [1, 3, 1, -1], 200), fr(12, [2, 3], 300)], "seg_ref_frame_ids": {0: [10, 11], 1: [12]}, "start_sid": 0}


def test_point_table_hand_written():
    m = _hand_map()
    s = _store(m)
    assert s.pt_ids.tolist() == [1, 2, 3, 7]
    # the FIRST row in store order: point 1 -> frame 10 row 0, 2 -> frame 10 row 1, 3 -> frame 11 row 1, 7 -> frame 10 row 3
    assert s.pt_xyz[:, 0].tolist() == [100.0, 101.0, 201.0, 103.0] and s.pt_desc[:, 0].tolist() == [100.0, 101.0, 201.0, 103.0]
    assert s.pt_sid.tolist() == [10, 11, 21, 13]
    _same_table(s, PJ.point_table(m))
    # explicit dicts override the rows, point by point; ids outside the table are passed over
    xy, de, si = {2: [9.0, 8.0, 7.0], 555: [0.0, 0.0, 0.0]}, {3: np.full(128, 0.5, np.float32)}, {1: 42, 7: 43}
    s2 = _store(m, point3D_xyzs=xy, point3D_descriptors=de, point3D_sids=si)
    assert s2.pt_xyz[1].tolist() == [9.0, 8.0, 7.0] and s2.pt_xyz[0, 0] == 100.0 and (s2.pt_desc[2] == 0.5).all() and s2.pt_desc[0, 0] == 100.0
    assert s2.pt_sid.tolist() == [42, 11, 21, 43]
    _same_table(s2, PJ.point_table(m, xy, de, si))
    # a point with a frame list and no row: covered by the dicts, or a ValueError
    m9 = dict(m, point3D_frame_ids={1: [10, 11, 11], 2: [10, 12], 3: [11, 12], 7: [10], 9: [12, 10], -1: [10]})
    full = dict(point3D_xyzs={9: [1.0, 2.0, 3.0]}, point3D_descriptors={9: np.ones(128, np.float32)}, point3D_sids={9: 5})
    s9 = _store(m9, **full)
    assert s9.pt_ids.tolist() == [1, 2, 3, 7, 9] and s9.pt_xyz[4].tolist() == [1.0, 2.0, 3.0] and s9.pt_sid[4] == 5 and s9.pt_desc[4, 7] == 1.0
    _same_table(s9, PJ.point_table(m9, full["point3D_xyzs"], full["point3D_descriptors"], full["point3D_sids"]))
    for missing in full:
        with pytest.raises(ValueError):
            _store(m9, **{k: v for k, v in full.items() if k != missing})
    with pytest.raises(ValueError):
        PJ.point_table(m9)
    # without any of the three arguments the table still votes; the values are refused where they are asked for
    lazy = _store(m9)
    assert lazy.pt_ids.tolist() == [1, 2, 3, 7, 9]
    with pytest.raises(ValueError):
        lazy.pt_xyz


def _zero_solver(k, x):
    return {"success": False, "inliers": np.zeros(len(k), bool)}


def _results(threshold=PJ.THRESHOLD, n_cov=RR.COVIS, solver=_zero_solver):
    map_, queries, planted, located = PJ.projection_scene()
    graph, table = RR.covisibility_graph(map_, n_cov), PJ.point_table(map_)
    out = []
    for l in located:
        if l is None:
            out.append(None)
            continue
        cam = planted[l["query"]]["cam"]
        out.append((l, cam, PJ.refine_by_projection(queries[l["query"]], map_, l, cam, solver, threshold=threshold, covisibility_frame=n_cov, graph=graph,
                                                    table=table)))
    return out


def test_restatement_reproduces_the_reference(golden):
    """Pinned by execution: the reference's refine_pose_by_projection was run on projection_scene with a recorder in place of
    pycolmap's solver; the restatement finds the same union, the same frustum mask, hands the solver the same rows and finds the
    same frames.  Reference frames inside and outside their own covisible list are both there."""
    g = golden("refine_projection_pinned")
    assert int(g["seed"]) == PJ.SCENE_SEED and float(g["threshold"]) == PJ.THRESHOLD and int(g["covisibility_frame"]) == RR.COVIS
    pattern = lambda k, x: {"success": True, "inliers": np.arange(len(k)) % 3 != 0}
    res = _results(solver=pattern)
    cases = g["cases"].tolist()
    assert cases == [i for i, r in enumerate(res) if r is not None]
    listed = set()
    for i in cases:
        l, cam, r = res[i]
        assert g[f"case{i}_query"][:2].tolist() == [l["query"], l["reference_frame_id"]]
        listed.add(int(g[f"case{i}_query"][2]))
        assert len(r["union"]) == int(g[f"case{i}_n_union"]), i
        assert np.array_equal(r["mask"].astype(np.uint8), g[f"case{i}_mask"]), i
        assert np.array_equal(r["matched_keypoint_ids"], g[f"case{i}_kpt_ids"]), i
        assert np.array_equal(r["matched_point3D_ids"], g[f"case{i}_point_ids"]), i
        assert np.array_equal(r["matched_sids"], g[f"case{i}_sids"]), i
        assert list(r["refinement_reference_frame_ids"]) == g[f"case{i}_best"].tolist(), i
    assert listed == {0, 1}


@pytest.mark.parametrize("n_cov", [RR.COVIS, 1])
def test_scene_margins(n_cov):
    """No decision of the scene the GPU tests use stands near its bound: pixel errors 1e-6 from 2 * threshold, u / v / depth 1e-6
    from a frustum bound, d0 / d1 1e-4 from 0.995, in-range distances 1e-5 apart.  n_cov = 1: the lists cut to one frame."""
    res = _results(n_cov=n_cov)
    enough = 0
    for i, x in enumerate(res):
        if x is None:
            continue
        l, cam, r = x
        m = PJ.margins(r, cam, PJ.THRESHOLD)
        print(f"projection scene, n_cov {n_cov}, entry {i} (query {l['query']}, frame {l['reference_frame_id']}): union {len(r['union'])}, in the "
              f"frustum {len(r['cand'])}, {len(r['matched_keypoint_ids'])} matches; margins {m}")
        assert m["range"] > 1e-6 and m["frustum"] > 1e-6 and m["ratio"] > 1e-4 and m["gap"] > 1e-5, (i, m)
        enough += l["enable"] and len(r["matched_keypoint_ids"]) >= 64
        # the matches are the planted ones: a matched keypoint that belongs to the pool matched its own point
        pool = queries_pool(l["query"])[r["matched_keypoint_ids"]]
        own = pool >= 0
        assert own.sum() >= 0.8 * len(pool)
    if n_cov == RR.COVIS:
        assert enough >= 3, enough      # three entries of the batch hand the solver 64 matches or more


_POOL = {}


def queries_pool(b):
    if not _POOL:
        _, queries, _ = RR.covisible_scene(PJ.SCENE_SEED)
        _POOL.update({i: q["pool"] for i, q in enumerate(queries)})
    return _POOL[b]


def test_gated_equals_dense_on_the_restatement():
    """The argument of DESIGN.md 4.14 on numbers: taking the two smallest distances among the in-range candidates only, and
    accepting a keypoint with exactly one of them, gives the dense formula's decisions."""
    for x in _results():
        if x is None:
            continue
        _, _, r = x
        dm = r["dm"]
        if "dist" not in dm:
            continue
        inr = dm["err"] < 2 * PJ.THRESHOLD
        plain = np.where(inr, dm["dist"] - np.where(inr, 0, 100).astype(np.float32), np.inf).astype(np.float32)      # in-range distances, no penalty
        order = np.argsort(plain, axis=1, kind="stable")[:, :2]
        d = np.take_along_axis(plain, order, 1)
        n_in = inr.sum(1)
        with np.errstate(all="ignore"):
            accept = (n_in == 1) | ((n_in >= 2) & (d[:, 0] / d[:, 1] <= np.float32(0.995)))
        assert np.array_equal(accept, dm["ratio_mask"])
        assert np.array_equal(order[n_in >= 1, 0], dm["ids"][n_in >= 1])
        assert {0, 1, 2} <= set(np.minimum(n_in, 2).tolist()) or len(n_in) < 20


def test_method_switch_rejects_unknown():
    from pram_amd.localization.refine import localize_and_refine
    with pytest.raises(NotImplementedError):
        localize_and_refine({}, None, None, None, None, seg_k=1, min_kpts=1, threshold=1.0, min_inliers=1, refinement_method="bundle")


def test_image_size_table():
    from pram_amd.localization.refine import image_size_table
    t = image_size_table(PR.PLANTED_CAMERAS)
    assert t.dtype == np.int32 and t.shape == (len(PR.PLANTED_CAMERAS), 2) and t[0].tolist() == [640, 480]


@pytest.mark.parametrize("n_points", [1, 31, 32, 33, 1000])
def test_mark_map_margins(n_points):
    """The crafted map of the GPU mark / project test: the store's tables equal the restatement's, and no projected point stands
    within 1e-6 of a frustum bound."""
    map_, queries = PJ.mark_map(n_points, 40 + n_points)
    store = _store(map_, covisibility_frame=4)
    table = PJ.point_table(map_)
    assert len(table["ids"]) == n_points
    _same_table(store, table)
    for n_cov in (4, 2):
        for q, w in zip(queries, PJ.mark_expected(map_, queries, n_cov, table)):
            if w is None:
                continue
            m = PJ.margins({"dm": {"err": np.zeros(0), "n_in": np.zeros(0, int)}, "u": w["u"], "v": w["v"], "depth": w["depth"]}, q["cam"], 1.0)
            assert m["frustum"] > 1e-6, (n_cov, q["reference_frame_id"], m)


@pytest.mark.parametrize("roll", [0, 4])
def test_match_case_margins(roll):
    """The crafted inputs of the GPU match test (seed 10): every decision stands clear of its bound."""
    case = PJ.match_case(10, roll)
    worst = {}
    for dm in PJ.match_expected(case):
        for k, v in PJ.match_margins(dm, case["threshold"]).items():
            worst[k] = min(worst.get(k, np.inf), v)
    print(f"match case, roll {roll}: margins {worst}")
    assert worst["range"] > 1e-6 and worst["ratio"] > 1e-4 and worst["gap"] > 1e-5, worst
