"""CPU: MultiMapStore's host layout against the maps it was composed of, its ValueErrors, the multi-map restatement
(tests/multimap_ref.py) against what the reference's own MultiMap3D.run decided (tests/golden/multimap_pinned.npz), and the new
entry's declaration."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import multimap_ref as MR
from tests import refine_ref as RR

ROOT = Path(__file__).resolve().parents[1]


def test_plan_maps_symbol_declared_and_exported(hip_lib):
    from pram_amd import _lib
    n = "pram_cand_plan_maps"
    assert n in _lib.exported_symbols()      # declared, typed and exported: tests/test_abi_contract_cpu.py
    # pram_cand_plan's argument list with the start_sid int replaced by a pointer
    one, many = _lib._SIGS["pram_cand_plan"], _lib._SIGS[n]
    assert many[0] is one[0] and len(many[1]) == len(one[1])
    assert [i for i, (a, b) in enumerate(zip(one[1], many[1])) if a is not b] == [13] and many[1][13] is _lib.P


def test_restatement_reproduces_the_reference(golden):
    """Per query and candidate: the sub-map, the in-map id, the query keypoints and the semantic flag MultiMap3D.run handed to
    localize_with_ref_frame."""
    g = golden("multimap_pinned")
    maps = MR.two_maps()
    cases = MR.pinned_cases(maps)
    assert int(g["n_queries"]) == len(cases) and g["names"].tolist() == list(MR.TWO_NAMES)
    assert int(g["seg_k"]) == MR.TWO_SEG_K and int(g["min_kpts"]) == MR.TWO_MIN_KPTS
    seen = set()
    for b, q in enumerate(cases):
        cs = MR.candidates(MR.real(q), maps, seg_k=MR.TWO_SEG_K, min_kpts=MR.TWO_MIN_KPTS)
        assert [c["map"] for c in cs] == g[f"q{b}_scene"].tolist(), b
        assert [c["lsid"] for c in cs] == g[f"q{b}_lsid"].tolist(), b
        assert [int(c["semantic_matching"]) for c in cs] == g[f"q{b}_semantic"].tolist(), b
        for w, c in enumerate(cs):
            assert np.array_equal(c["q_kpt_ids"], g[f"q{b}_c{w}_kpt_ids"]), (b, w)
            assert c["sid"] == c["lsid"] + maps[c["map"]]["start_sid"]
            seen.add((c["map"], c["semantic_matching"]))
            if c["semantic_matching"] and c["lsid"] == 0:      # the sid > 0 rule, per map: the whole frame
                assert len(c["ref_rows"]) == maps[c["map"]]["frames"][c["reference_frame"]]["keypoints"].shape[0]
                seen.add(("sid0", c["map"]))
    assert [c["map"] for c in MR.candidates(MR.real(cases[0]), maps, seg_k=6, min_kpts=8)] == [0, 1, 0, 1, 0, 1]
    assert seen == {(0, False), (0, True), (1, False), (1, True), ("sid0", 0), ("sid0", 1)}, seen


def test_restatement_landmark_nobody_owns():
    maps = MR.two_maps()
    maps[1] = dict(maps[1], start_sid=12)      # a gap: global ids 10 and 11
    assert MR.owner(maps, 9) == (0, 9) and MR.owner(maps, 10) is None and MR.owner(maps, 12) == (1, 0) and MR.owner(maps, 20) is None
    q = MR._join(5, [maps[0], dict(maps[1], start_sid=10)], ([(0, 16)], [(1, 12)]), 4, n_class=21)      # votes for 0 and for 11
    cs = MR.candidates(MR.real(q), maps, seg_k=2, min_kpts=8)
    assert [c["sid"] for c in cs] == [0, 11] and cs[0]["map"] == 0 and cs[1]["map"] is None and cs[1]["store_frame"] == -1
    assert len(cs[1]["q_kpt_ids"]) == 0 and len(cs[1]["ref_rows"]) == 0


def _stores(maps, **kw):
    from pram_amd.localization.candidates import ReferenceStore
    return [ReferenceStore(m["frames"], m["seg_ref_frame_ids"], m["start_sid"], **kw) for m in maps]


def _csr(off, vals, i):
    return vals[off[i]:off[i + 1]]


@pytest.mark.parametrize("scene", ["two_maps", "twin_maps"])
def test_host_layout(scene):
    """Every row, frame, histogram, landmark slice, point list and covisible list of map m is found at its offset."""
    from pram_amd.localization.multimap import MultiMapStore
    if scene == "two_maps":
        maps, names, parts = MR.two_maps(), MR.TWO_NAMES, _stores(MR.two_maps(), covisibility_frame=3)
    else:
        maps, names = MR.twin_maps()[0], MR.TWIN_NAMES
        parts = _stores(maps, covisibility_frame=RR.COVIS)
    S = MultiMapStore(parts, names)
    assert S.n_maps == 2 and S.names == list(names) and S.start_sid == 0 and S.covisibility_frame == parts[0].covisibility_frame
    assert S.n_frames == sum(p.n_frames for p in parts) and S.n_rows == sum(p.n_rows for p in parts)
    assert S.max_frame_rows == max(p.max_frame_rows for p in parts)
    assert len(S.lm_frame) == len(S.lm_start) == max(p.start_sid + len(p.lm_frame) for p in parts)
    assert np.all(np.diff(S.pt_ids) > 0) and S.pt_ids.dtype == np.int64 and S.point3D_ids.dtype == np.int64
    F0 = R0 = P0 = 0
    for m, p in enumerate(parts):
        assert S.map_frame_off[m] == F0 and S.map_row_off[m] == R0
        for f in range(p.n_frames):
            g = F0 + f
            assert S.frame_ids[g] == (names[m], p.frame_ids[f]) and S.frame_map[g] == m and S.scene_of(g) == names[m]
            assert np.array_equal(S.rows(g), p.rows(f) + R0)
            rows, prow = S.rows(g), p.rows(f)
            for name in ("keypoints", "scores", "descriptors", "xyzs", "keypoint_segs"):
                assert np.array_equal(getattr(S, name)[rows], getattr(p, name)[prow]), name
            sm, raw = S.split_point_ids(S.point3D_ids[rows])
            assert np.array_equal(raw, p.point3D_ids[prow]) and np.array_equal(sm, np.where(raw < 0, -1, m))
            assert np.array_equal(S.frame_norm[g], p.frame_norm[f]) and np.array_equal(S.frame_size[g], p.frame_size[f]) and S.is_vrf[g] == p.is_vrf[f]
            assert np.array_equal(_csr(S.hist_off, S.hist_label, g), _csr(p.hist_off, p.hist_label, f))      # in-map labels
            assert np.array_equal(_csr(S.hist_off, S.hist_cnt, g), _csr(p.hist_off, p.hist_cnt, f))
            assert np.array_equal(S.covisible(g), p.covisible(f) + F0)
            assert np.array_equal(_csr(S.covis_off, S.covis_count, g), _csr(p.covis_off, p.covis_count, f))
            for sid in np.unique(p.keypoint_segs[prow]).tolist() + [9999]:
                assert np.array_equal(S.rows_by_sid(g, sid), p.rows_by_sid(f, sid) + R0)
        for l in range(len(p.lm_frame)):
            G = p.start_sid + l
            assert S.lm_start[G] == p.start_sid and S.lm_sel_len[G] == p.lm_sel_len[l]
            assert S.lm_frame[G] == (p.lm_frame[l] + F0 if p.lm_frame[l] >= 0 else -1)
            sel = S.sel_rows[S.lm_sel_off[G]:S.lm_sel_off[G] + S.lm_sel_len[G]]
            assert np.array_equal(sel, p.sel_rows[p.lm_sel_off[l]:p.lm_sel_off[l] + p.lm_sel_len[l]] + R0)
            if p.lm_frame[l] >= 0:
                assert np.array_equal(sel, S.rows_by_sid(int(S.lm_frame[G]), l))
        n = len(p.pt_ids)
        assert S.map_point_off[m] == P0
        assert np.array_equal(S.pt_ids[P0:P0 + n], S.store_point_ids(m, p.pt_ids))
        for i in range(n):
            assert np.array_equal(_csr(S.pt_off, S.pt_frames, P0 + i), _csr(p.pt_off, p.pt_frames, i) + F0)
        for name in ("pt_xyz", "pt_desc", "pt_sid"):
            assert np.array_equal(getattr(S, name)[P0:P0 + n], getattr(p, name)), name
        F0, R0, P0 = F0 + p.n_frames, R0 + p.n_rows, P0 + n
    owned = np.zeros(len(S.lm_frame), bool)
    for p in parts:
        owned[p.start_sid:p.start_sid + len(p.lm_frame)] = True
    assert (S.lm_frame[~owned] == -1).all()
    # the raw ids of the two maps intersect; the store's do not
    raw = [np.unique(p.pt_ids) for p in parts]
    assert np.intersect1d(*raw).size > 0 and len(np.unique(S.pt_ids)) == sum(len(r) for r in raw)


def test_point_id_round_trip():
    from pram_amd.localization.multimap import MultiMapStore as M
    raw = np.array([0, 1, 5, 2 ** 40 - 1, 123456789012], dtype=np.int64)
    for m in (0, 1, 6, 1000):
        ids = M.store_point_ids(m, raw)
        sm, back = M.split_point_ids(ids)
        assert ids.dtype == np.int64 and np.array_equal(back, raw) and (sm == m).all()
        tm, tb = M.split_point_ids(torch.from_numpy(ids))
        assert torch.equal(tb, torch.from_numpy(raw)) and bool((tm == m).all()) and torch.equal(M.store_point_ids(m, torch.from_numpy(raw)), torch.from_numpy(ids))
        if m:
            assert (ids > M.store_point_ids(m - 1, raw).max()).all()      # monotone in (map, id)
    both = np.array([-1, 7, -1], dtype=np.int64)
    assert M.store_point_ids(3, both).tolist() == [-1, 7 | 3 << 40, -1]
    assert [x.tolist() for x in M.split_point_ids(M.store_point_ids(3, both))] == [[-1, 3, -1], [-1, 7, -1]]
    assert [x.tolist() for x in M.split_point_ids(torch.tensor([-1, 7 | 3 << 40]))] == [[-1, 3], [-1, 7]]
    # a map index per id
    assert M.store_point_ids(np.array([0, 2]), np.array([9, 9])).tolist() == [9, 9 | 2 << 40]


_ARRAYS = ("keypoints", "scores", "descriptors", "xyzs", "point3D_ids", "keypoint_segs", "frame_size", "frame_norm", "frame_off", "sel_rows",
           "hist_label", "hist_cnt", "hist_off", "lm_frame", "lm_sel_off", "lm_sel_len", "pt_ids", "pt_off", "pt_frames", "is_vrf", "covis_off",
           "covis_frames", "covis_count", "pt_xyz", "pt_desc", "pt_sid")


def test_single_map_equals_the_map():
    from pram_amd.localization.multimap import MultiMapStore
    m = RR.covisible_scene()[0]
    A = _stores([m], covisibility_frame=RR.COVIS)[0]
    S = MultiMapStore([A], ["only"])
    for name in _ARRAYS:
        a, s = getattr(A, name), getattr(S, name)
        assert a.dtype == s.dtype and a.shape == s.shape and np.array_equal(a, s), name
    assert not S.lm_start.any() and S.frame_ids == [("only", fid) for fid in A.frame_ids]
    assert (S.n_frames, S.n_rows, S.max_frame_rows) == (A.n_frames, A.n_rows, A.max_frame_rows)
    # the map further up in the numbering: its landmark tables move, nothing else does
    A4 = _stores([dict(m, start_sid=4)], covisibility_frame=RR.COVIS)[0]
    S4 = MultiMapStore([A4], ["only"])
    assert len(S4.lm_frame) == 4 + len(A.lm_frame) and (S4.lm_frame[:4] == -1).all()
    for name in ("lm_frame", "lm_sel_off", "lm_sel_len"):
        assert np.array_equal(getattr(S4, name)[4:], getattr(A, name)), name
    assert (S4.lm_start[4:] == 4).all() and S4.start_sid == 0
    for name in _ARRAYS:
        if not name.startswith("lm_"):
            assert np.array_equal(getattr(S4, name), getattr(A, name)), name


def test_value_errors():
    from pram_amd.localization.candidates import ReferenceStore
    from pram_amd.localization.multimap import MultiMapStore
    a, b = MR.two_maps()
    sa, sb = _stores([a, b])
    MultiMapStore([sa, sb], ["x", "y"])
    with pytest.raises(ValueError, match="no map"):
        MultiMapStore([], [])
    with pytest.raises(ValueError, match="unique"):
        MultiMapStore([sa, sb], ["x", "x"])
    with pytest.raises(ValueError, match="overlap"):      # 10 landmarks from 0 and 8 from 9
        MultiMapStore([sa, _stores([dict(b, start_sid=9)])[0]], ["x", "y"])
    with pytest.raises(ValueError, match="overlap"):      # in either order
        MultiMapStore([_stores([dict(b, start_sid=2)])[0], sa], ["y", "x"])
    with pytest.raises(ValueError, match="covisibility_frame"):
        MultiMapStore([sa, _stores([b], covisibility_frame=5)[0]], ["x", "y"])
    for bad in (-2, 2 ** 40):
        fr = [dict(f) for f in b["frames"]]
        fr[1]["point3D_ids"] = fr[1]["point3D_ids"].copy()
        fr[1]["point3D_ids"][3] = bad
        with pytest.raises(ValueError, match="point id"):
            MultiMapStore([sa, ReferenceStore(fr, b["seg_ref_frame_ids"], b["start_sid"])], ["x", "y"])
    fr = [dict(f) for f in b["frames"]]
    fr[1]["point3D_ids"] = fr[1]["point3D_ids"].copy()
    fr[1]["point3D_ids"][3] = 2 ** 40 - 1      # the largest raw id
    MultiMapStore([sa, ReferenceStore(fr, b["seg_ref_frame_ids"], b["start_sid"])], ["x", "y"])
    # a gap between the ranges is no error: nobody's landmarks
    S = MultiMapStore([sa, _stores([dict(b, start_sid=13)])[0]], ["x", "y"])
    assert (S.lm_frame[10:13] == -1).all() and len(S.lm_frame) == 21


def test_per_point_values_are_checked_on_first_use():
    """ReferenceStore's rule, per map: a vote-only point table composes; the values raise where they are first asked for."""
    from pram_amd.localization.candidates import ReferenceStore
    from pram_amd.localization.multimap import MultiMapStore
    a, b = MR.two_maps()
    sa = _stores([a])[0]
    p2f = {int(p): [100] for p in np.concatenate([f["point3D_ids"] for f in b["frames"]])}
    p2f[777777] = [101]      # a point without a row
    sb = ReferenceStore(b["frames"], b["seg_ref_frame_ids"], b["start_sid"], point3D_frame_ids=p2f)
    S = MultiMapStore([sa, sb], ["x", "y"])
    assert S.store_point_ids(1, 777777) in S.pt_ids
    with pytest.raises(ValueError, match="neither a value nor a row"):
        S.pt_xyz


def test_stores_share_the_base_and_the_host_views():
    """Both stores derive from StoreBase (MultiMapStore is no ReferenceStore) and take every shared method from it; a one-map
    store answers the host views as the map does."""
    from pram_amd.localization.candidates import ReferenceStore, StoreBase
    from pram_amd.localization.multimap import MultiMapStore
    assert issubclass(ReferenceStore, StoreBase) and issubclass(MultiMapStore, StoreBase) and not issubclass(MultiMapStore, ReferenceStore)
    for name in ("tables", "point_tables", "covisible", "rows", "rows_by_sid", "n_frames", "n_rows", "max_frame_rows", "pt_xyz", "pt_desc", "pt_sid"):
        assert name not in vars(ReferenceStore) and name not in vars(MultiMapStore) and name in vars(StoreBase), name
    assert "_point_values" in vars(ReferenceStore) and "_point_values" in vars(MultiMapStore)
    assert MultiMapStore._EXTRA_PADDED == ("lm_start",) and MultiMapStore._EXTRA_COUNTS == ("n_maps",) and ReferenceStore._EXTRA_PADDED == ()
    m = RR.covisible_scene()[0]
    one = _stores([dict(m, start_sid=0)], covisibility_frame=RR.COVIS)[0]
    S = MultiMapStore([one], ["only"])
    assert (S.n_frames, S.n_rows, S.max_frame_rows) == (one.n_frames, one.n_rows, one.max_frame_rows) and S.n_maps == 1
    for f in range(one.n_frames):
        assert np.array_equal(S.rows(f), one.rows(f)) and np.array_equal(S.covisible(f), one.covisible(f))
        for sid in np.unique(one.keypoint_segs[one.rows(f)]).tolist() + [9999]:
            assert np.array_equal(S.rows_by_sid(f, sid), one.rows_by_sid(f, sid))
    for name in ("pt_xyz", "pt_desc", "pt_sid"):
        assert np.array_equal(getattr(S, name), getattr(one, name)) and getattr(S, name).dtype == getattr(one, name).dtype
    from pram_amd._lib import PramHipError
    for store in (one, S):
        with pytest.raises(PramHipError):
            store.tables("cpu")
