"""GPU: map compression on the device (pram_amd.localization.compress, csrc/compress.hip) against the numpy restatement
tests/compress_ref.py and the fixture pinned by the reference on the shared scene, the selection and sparsification kernels on
hand-made cases whose arithmetic is exact, the compressed store, and the C entries' refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import compress_ref as CR
from tests import helpers as H

pytestmark = pytest.mark.gpu

W, HGT, FOCAL = 640.0, 480.0, 512.0
CAM = [1.0, 0, 0, 0, 0, 0, 0, FOCAL, FOCAL, 0, 0, W, HGT]      # identity pose, no principal point: a point (u / 512, v / 512, 1) lands on (u, v) exactly


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.shape[0] else np.zeros((1,) + a.shape[1:], dtype=a.dtype)).to(dev)


# ------------------------------------------------------------------------------------------------ the whole scene
@pytest.fixture(scope="module")
def run(dev):
    """compress_map on the scene for the three configurations, twice each; the stores are kept for the later tests."""
    from pram_amd.localization import compress as CP
    from pram_amd.localization.candidates import ReferenceStore
    s = CR.scene()
    frames = CR.store_frames(s)
    out = {"scene": s, "stores": {}}
    vrf = [CR.FRAME_ID0 + f for f in CR.vrf_order(s["seg_ref"], 1)]
    assert CP.vrf_order(CR.store_arguments(s, 5)["seg_ref_frame_ids"], 1) == vrf
    for n in (5, 30):
        out["stores"][n] = ReferenceStore(frames, **CR.store_arguments(s, n))
        assert np.array_equal(out["stores"][n].pt_ids, s["pt_ids"])
    for tag, cfg in CR.CONFIGS.items():
        store = out["stores"][cfg["covisible_frames"]]
        for again in ("", "_again"):
            out[tag + again] = CP.compress_map(store, s["cams"], vrf, radius=CR.RADIUS, nkpts=cfg["nkpts"], xys=s["xys"],
                                               point3D_obs={int(p): int(o) for p, o in zip(s["pt_ids"], s["pt_obs"])}, device=dev)
    return out


@pytest.mark.parametrize("tag", list(CR.CONFIGS))
def test_scene_equals_restatement_and_reference(run, golden, tag):
    got, want, g = run[tag], run["scene"]["results"][tag], golden("compress_pinned")
    frames = [fid - CR.FRAME_ID0 for fid in got["frame_ids"]]
    assert frames == want["frames"] == g[tag + "_frames"].tolist()
    off, ids = g[tag + "_list_off"], g[tag + "_list_ids"]
    for i, f in enumerate(frames):
        mine = got["frame_point_ids"][CR.FRAME_ID0 + f]
        assert mine.dtype == np.int64 and np.array_equal(mine, want["lists"][f]) and np.array_equal(mine, ids[off[i]:off[i + 1]]), (tag, f)
    assert list(got["point3D_frame_ids"]) == list(want["point_frames"]) == g[tag + "_pt_ids"].tolist() == got["point_ids"].tolist()
    off, pf = g[tag + "_pt_off"], g[tag + "_pt_frames"]
    for i, p in enumerate(got["point_ids"].tolist()):
        mine = [fid - CR.FRAME_ID0 for fid in got["point3D_frame_ids"][p]]
        assert mine == want["point_frames"][p] == pf[off[i]:off[i + 1]].tolist(), (tag, p)


def test_two_runs_are_bit_equal(run):
    for tag in CR.CONFIGS:
        a, b = run[tag], run[tag + "_again"]
        assert a["frame_ids"] == b["frame_ids"] and np.array_equal(a["point_ids"], b["point_ids"])
        assert all(np.array_equal(a["frame_point_ids"][f], b["frame_point_ids"][f]) for f in a["frame_ids"])
        assert a["point3D_frame_ids"] == b["point3D_frame_ids"]


def test_default_keypoints_are_the_stores(run, dev):
    """Without ``xys`` the store's float32 keypoints are widened: the restatement on the same numbers."""
    from pram_amd.localization import compress as CP
    s, store = run["scene"], run["stores"][5]
    vrf = CR.vrf_order(s["seg_ref"], 1)
    got = CP.compress_map(store, s["cams"], [CR.FRAME_ID0 + f for f in vrf], radius=CR.RADIUS, device=dev)
    s32 = {**s, "xys": s["xys"].astype(np.float32).astype(np.float64)}
    want = CR.compress(s32, 5, -1)
    assert [fid - CR.FRAME_ID0 for fid in got["frame_ids"]] == want["frames"]
    assert all(np.array_equal(got["frame_point_ids"][CR.FRAME_ID0 + f], want["lists"][f]) for f in want["frames"])


# ------------------------------------------------------------------------------------------------ the selection kernels, directly
def _select(dev, frames, points, covis, vrf, radius=20.0, cov=4, cams=None):
    """frames: per frame a list of (point id, (kx, ky)); points: point id -> xyz; covis: frame -> candidates; vrf: frames in order
    -> (retained order per frame, per frame the kept point ids)."""
    from pram_amd import ops
    F = len(frames)
    frame_off = np.zeros(F + 1, dtype=np.int32)
    frame_off[1:] = np.cumsum([len(f) for f in frames])
    ids = np.array([p for f in frames for p, _ in f], dtype=np.int64)
    xys = np.array([k for f in frames for _, k in f], dtype=np.float64).reshape(-1, 2)
    pt_ids = np.array(sorted(points), dtype=np.int64)
    pt_xyz = np.array([points[p] for p in pt_ids.tolist()], dtype=np.float64).reshape(-1, 3)
    covis_off = np.zeros(F + 1, dtype=np.int32)
    covis_off[1:] = np.cumsum([len(covis.get(f, [])) for f in range(F)])
    covis_frames = np.array([c for f in range(F) for c in covis.get(f, [])], dtype=np.int32)
    cams = np.array([CAM] * F, dtype=np.float64) if cams is None else cams
    store = {"point3D_ids": _up(ids, dev), "frame_off": _up(frame_off, dev), "pt_ids": _up(pt_ids, dev), "n_frames": F, "n_rows": len(ids),
             "n_points": len(pt_ids), "covisibility_frame": cov}
    order, cnt, lst = ops.compress_select(store, frame_off, covis_off, covis_frames, np.array(vrf, dtype=np.int32), _up(pt_xyz, dev), _up(xys, dev),
                                          _up(cams, dev), radius)
    order, cnt, lst = order.cpu().numpy(), cnt.cpu().numpy(), lst.cpu().numpy()
    return order.tolist(), [pt_ids[lst[frame_off[f]:frame_off[f] + cnt[f]]].tolist() for f in range(F)]


def _at(u, v, z=1.0):
    return [u * z / FOCAL, v * z / FOCAL, z]


def test_select_radius_is_inclusive(dev):
    """A keypoint at offset (12, 16) from the projection is exactly 20 away: discarded; one ulp further: kept."""
    points = {1: _at(0, 0), 2: _at(100, 100), 3: _at(300, 300)}
    for ky, kept in ((116.0, [3]), (np.nextafter(116.0, np.inf), [2, 3]), (np.nextafter(116.0, -np.inf), [3])):
        order, lists = _select(dev, [[(1, (112.0, ky))], [(2, (0.0, 0.0)), (3, (0.0, 0.0))]], points, {0: [0, 1]}, [0])
        assert order == [0, 1] and lists == [[1], kept], ky
    # the same through the other coordinate and on the far side
    order, lists = _select(dev, [[(1, (84.0, 88.0))], [(2, (0.0, 0.0)), (3, (0.0, 0.0))]], points, {0: [1]}, [0])
    assert lists[1] == [3]


def test_select_depth_and_image_tests(dev):
    """p_z <= 0 and a projection outside the image keep the row, whatever keypoint lies beside it; the borders are 0 <= u < w."""
    points = {1: _at(0, 0), 10: [-100 / FOCAL, -100 / FOCAL, -1.0], 11: [100 / FOCAL, 100 / FOCAL, 0.0], 12: _at(-5, 100), 13: _at(640, 100),
              14: _at(0, 100), 15: _at(100, 480), 16: _at(100, 0), 17: _at(639.5, 479.5)}
    vrf_rows = [(1, (100.0, 100.0)), (1, (-3.0, 100.0)), (1, (640.0, 100.0)), (1, (0.0, 100.0)), (1, (100.0, 480.0)), (1, (100.0, 0.0)), (1, (639.5, 479.5))]
    cand = [(p, (1.0, 1.0)) for p in (10, 11, 12, 13, 14, 15, 16, 17)]
    order, lists = _select(dev, [vrf_rows, cand], points, {0: [0, 1]}, [0])
    assert order == [0, 1] and lists[1] == [10, 11, 12, 13, 15]      # 14, 16 and 17 lie inside, on a keypoint


def test_select_chain_rules(dev):
    """A chain frame without kept keypoints; a candidate that loses every row; a candidate equal to the reference frame; a
    discarded row's keypoint, an id -1 row's and an unknown id's discard nothing; a kept row of a candidate does."""
    # frame 0: no valid row at all -> retained, empty, discards nothing
    points = {2: _at(100, 100)}
    order, lists = _select(dev, [[(-1, (100.0, 100.0)), (77, (100.0, 100.0))], [(2, (5.0, 5.0))]], points, {0: [0, 1]}, [0])
    assert order == [0, 1] and lists == [[], [2]]
    # frame 1 loses its only row: not retained, and frame 2 is not tested against it (its keypoint lies on frame 2's projection)
    points = {1: _at(100, 100), 2: _at(100, 100), 3: _at(400, 400)}
    order, lists = _select(dev, [[(1, (100.0, 100.0))], [(2, (400.0, 400.0))], [(3, (9.0, 9.0))]], points, {0: [1, 0, 2]}, [0])
    assert order == [0, -1, 1] and lists == [[1], [], [3]]
    # frame 1: row B1 is discarded by frame 0, row B2 stays.  Frame 2: C lies on B1's keypoint (kept), D on B2's (discarded), E on
    # the keypoint of frame 0's id -1 row and G on that of its unknown id (kept)
    points = {1: _at(100, 100), 21: _at(100, 100), 22: _at(200, 200), 31: _at(300, 300), 32: _at(200, 200), 33: _at(500, 400), 34: _at(50, 400)}
    frames = [[(1, (100.0, 100.0)), (-1, (500.0, 400.0)), (999, (50.0, 400.0))], [(21, (300.0, 300.0)), (22, (200.0, 200.0))],
              [(31, (0.0, 0.0)), (32, (0.0, 0.0)), (33, (0.0, 0.0)), (34, (0.0, 0.0))]]
    order, lists = _select(dev, frames, points, {0: [0, 1, 2]}, [0])
    assert order == [0, 1, 2] and lists == [[1], [22], [31, 33, 34]]


def test_select_overwrite_order_and_repeats(dev):
    """A reference frame first retained in part keeps its place and gets every valid row back; a retained candidate joins the
    chain; a reference frame given twice is taken again."""
    points = {1: _at(100, 100), 21: _at(100, 100), 22: _at(200, 200), 31: _at(200, 200), 32: _at(100, 100), 33: _at(600, 20), 41: _at(600, 20)}
    frames = [[(1, (100.0, 100.0))], [(21, (100.0, 100.0)), (22, (200.0, 200.0)), (-1, (1.0, 1.0))], [(31, (9.0, 9.0)), (32, (9.0, 9.0)), (33, (600.0, 20.0))],
              [(41, (7.0, 7.0))]]
    # under 0: frame 1 keeps [22]; frame 2: 31 falls to frame 1's kept row, 32 to frame 0 -> [33]
    order, lists = _select(dev, frames, points, {0: [0, 1, 2], 1: [1, 2, 3]}, [0])
    assert order == [0, 1, 2, -1] and lists == [[1], [22], [33], []]
    # then 1 as a reference frame: all valid rows back, place 1 stays; 2 is retained already and joins the chain, so 41 falls to it
    order, lists = _select(dev, frames, points, {0: [0, 1, 2], 1: [1, 2, 3]}, [0, 1, 0])
    assert order == [0, 1, 2, -1] and lists == [[1], [21, 22], [33], []]
    # without frame 2 in the list, 41 meets nothing
    order, lists = _select(dev, frames, points, {0: [0, 1], 1: [1, 3]}, [0, 1])
    assert order == [0, 1, -1, 2] and lists == [[1], [21, 22], [], [41]]


def test_select_tiles(dev):
    """Rows and keypoints beyond the first tile of either kind: a candidate of 600 rows against a chain frame of 700 keypoints,
    where only the last keypoint of the chain frame covers the last row of the candidate."""
    n, m = 600, 700
    points = {1: _at(630, 470), 2: _at(10, 10)}
    vrf_rows = [(-1, (10.0, 10.0))] * (m - 1) + [(1, (10.0, 10.0))]      # id -1 rows on the spot: they must not count
    cand = [(2, (0.0, 0.0))] * n
    order, lists = _select(dev, [vrf_rows, cand], points, {0: [1]}, [0])
    assert order == [0, -1] and lists == [[1], []]
    points[3] = _at(630, 470)
    cand = [(3, (0.0, 0.0))] * (n - 1) + [(2, (0.0, 0.0))]
    order, lists = _select(dev, [vrf_rows, cand], points, {0: [1]}, [0])
    assert order == [0, 1] and lists == [[1], [3] * (n - 1)]


# ------------------------------------------------------------------------------------------------ sparsification, directly
def _sparsify(dev, uv, scores, nkpts, radius=20.0, xyz=None):
    from pram_amd import ops
    n = len(scores)
    xyz = np.array([_at(u, v) for u, v in uv], dtype=np.float64) if xyz is None else np.asarray(xyz, dtype=np.float64)
    frame_off = np.array([0, 3, 3 + n], dtype=np.int32)      # a frame listing one point first: the lists sit at the frames' offsets
    store = {"frame_off": _up(frame_off, dev), "n_frames": 2, "n_rows": 3 + n, "n_points": n, "covisibility_frame": 1}
    list_pt = _up(np.concatenate([[0, 1, 2], np.arange(n)]).astype(np.int32), dev)
    list_cnt = _up(np.array([1, n], dtype=np.int32), dev)
    ops.compress_sparsify(store, _up(np.array([CAM, CAM]), dev), _up(xyz, dev), _up(np.asarray(scores, dtype=np.int32), dev), radius, nkpts, list_pt, list_cnt)
    cnt, lst = list_cnt.cpu().numpy(), list_pt.cpu().numpy()
    assert cnt[0] == 1 and lst[:3].tolist() == [0, 1, 2]
    return lst[3:3 + cnt[1]].tolist()


def test_sparsify_rules(dev):
    uv = [(5, 5), (45, 5), (6, 6), (40.0, 30), (-3, 7), (7, 7), (59, 31), (39.999, 30), (-3, -41)]
    scores = [3, 1, 3, 2, 9, 4, 8, 1, 5]
    # cell (0, 0): 0 and 2 tie (the earlier holds), 5 beats both; 40.0 is cell 2, where 59 beats it; 39.999 is cell 1; negative cells
    want = [5, 1, 6, 4, 7, 8]
    assert _sparsify(dev, uv, scores, nkpts=8) == want
    xyz = np.array([_at(u, v) for u, v in uv])
    assert CR.sparsify(np.array(CAM), xyz, np.array(scores), 20.0)[0].tolist() == want
    assert _sparsify(dev, uv, scores, nkpts=9) == list(range(9))      # exactly nkpts points: untouched
    assert _sparsify(dev, uv, scores, nkpts=100) == list(range(9))
    # a tie between two cells' winners changes nothing; the order is the cells', not the winners'
    assert _sparsify(dev, [(5, 5), (25, 5), (6, 6)], [1, 1, 2], nkpts=1) == [2, 1]


def test_sparsify_drops_what_does_not_project_and_takes_long_lists(dev):
    xyz = [_at(5, 5), [0.1, 0.1, 0.0], _at(30, 5), [0.0, 0.0, 0.0]]      # z = 0: infinite and NaN projections
    assert _sparsify(dev, None, [1, 9, 1, 9], nkpts=1, xyz=xyz) == [0, 2]
    # 704 points on a lattice of 32 x 11 cells, each cell twice: the second visit has the higher score
    rng = np.random.default_rng(5)
    cells = rng.permutation(352)
    uv = [((c % 32) * 20 + 3.5, (c // 32) * 20 + 7.25) for c in cells] + [((c % 32) * 20 + 11.0, (c // 32) * 20 + 2.0) for c in cells[::-1]]
    scores = [1] * 352 + [2] * 352
    want = CR.sparsify(np.array(CAM), np.array([_at(u, v) for u, v in uv]), np.array(scores), 20.0)[0].tolist()
    assert want == [703 - i for i in range(352)]
    assert _sparsify(dev, uv, scores, nkpts=10) == want


# ------------------------------------------------------------------------------------------------ the compressed store
def test_compressed_store(run, dev):
    from pram_amd.localization import candidates as cd
    from pram_amd.localization import compress as CP
    from pram_amd.nets.gml import GML
    s, store, result = run["scene"], run["stores"][30], run["c30"]
    seg_ref = CR.store_arguments(s, 30)["seg_ref_frame_ids"]
    err = {int(p): float(e) for p, e in zip(s["pt_ids"], s["pt_err"])}
    held = result["point_ids"]
    swap = {CR.FRAME_ID0 + 8: [int(held[5]), int(np.setdiff1d(s["pt_ids"], held)[0]), int(held[2])]}      # original_points3d of frame 8
    cs = CP.compressed_store(store, result, seg_ref, err, vrf_point_ids=swap, device=dev, covisibility_frame=5)
    frames = [fid - CR.FRAME_ID0 for fid in result["frame_ids"]]
    assert cs.frame_ids == result["frame_ids"] and np.array_equal(cs.pt_ids, np.sort(held))
    for i, f in enumerate(frames):
        ids = [int(held[5]), int(held[2])] if f == 8 else result["frame_point_ids"][CR.FRAME_ID0 + f]
        want = CR.frame_rows(s, f, ids)
        a, b = cs.frame_off[i], cs.frame_off[i + 1]
        assert np.array_equal(cs.point3D_ids[a:b], want["point3D_ids"]) and np.array_equal(cs.xyzs[a:b], want["xyzs"])
        assert np.array_equal(cs.keypoints[a:b], want["keypoints"][:, :2].astype(np.float32)) and np.array_equal(cs.scores[a:b], want["keypoints"][:, 2].astype(np.float32))
        assert np.array_equal(cs.keypoint_segs[a:b], want["keypoint_segs"])
        assert np.array_equal(cs.descriptors[a:b], store.pt_desc[np.searchsorted(store.pt_ids, want["point3D_ids"])])
    # the float64 rows, before the store narrows them: bit-equal to the restatement
    f = frames[4]
    ids = result["frame_point_ids"][CR.FRAME_ID0 + f]
    rows = CP.project_rows(store, s["cams"], np.full(len(ids), f), np.searchsorted(store.pt_ids, ids), err, dev)
    assert np.array_equal(rows["keypoints"], CR.frame_rows(s, f, ids)["keypoints"])
    # a query made of the first 256 rows of the compressed frame 0 goes through match_candidates
    n = 256
    seg = np.zeros((1, n, len(seg_ref) + 1), dtype=np.float32)
    seg[0, np.arange(n), cs.keypoint_segs[:n] + 1] = 5.0
    feats = {"keypoints": torch.from_numpy(cs.keypoints[:n].copy())[None].to(dev), "scores": torch.from_numpy(cs.scores[:n].copy())[None].to(dev),
             "descriptors": torch.from_numpy(cs.descriptors[:n].copy())[None].to(dev), "counts": torch.tensor([n], dtype=torch.int32, device=dev),
             "image_size": (CR.WIDTH, CR.HEIGHT)}
    g = GML({})
    g.load_state_dict(H.gml_sd(), strict=True)
    g.precision = None
    out = cd.match_candidates(feats, torch.from_numpy(seg).to(dev), cs, g.to(dev).eval(), seg_k=2, min_kpts=8, semantic_matching=False)
    assert len(out) == 1 and len(out[0]) == 2
    live = [c for c in out[0] if c["reference_frame_id"] is not None]
    assert live and all(c["reference_frame_id"] in cs.frame_ids for c in live)
    for c in live:
        i = cs.frame_ids.index(c["reference_frame_id"])
        assert c["n_ref_kpts"] == cs.frame_off[i + 1] - cs.frame_off[i] and c["n_query_kpts"] == n
        assert bool(torch.isfinite(c["matching_scores0"]).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_c_entries_refuse_without_launching(run, dev, hip_lib):
    """A null pointer, a workspace that is too small, a reference frame without a covisible list, a misaligned buffer: PRAM_E_ARG and
    the outputs untouched; the same calls, complete, succeed."""
    L, s, store = hip_lib, run["scene"], run["stores"][5]
    t = store.point_tables(dev)
    F, n_rows = t["n_frames"], t["n_rows"]
    ints = lambda a: (C.c_int * max(len(a), 1))(*[int(x) for x in a])
    fo, co, cf = ints(store.frame_off), ints(store.covis_off), ints(store.covis_frames)
    vrf = ints(CR.vrf_order(s["seg_ref"], 1))
    xys, cams = _up(s["xys"], dev), _up(s["cams"], dev)
    need = L.pram_compress_workspace_bytes(n_rows, 5)
    assert need == 24 * n_rows + 4 * 6 + 16
    ws = torch.empty(need + 8, device=dev, dtype=torch.uint8)
    order = torch.full((F,), -77, device=dev, dtype=torch.int32)
    cnt = torch.full((F,), -77, device=dev, dtype=torch.int32)
    lst = torch.full((n_rows,), -77, device=dev, dtype=torch.int32)
    st = torch.cuda.current_stream().cuda_stream

    def select(ids=t["point3D_ids"].data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need, vrf=vrf, n_vrf=4, radius=20.0, out=lst.data_ptr(), cov=5):
        return L.pram_compress_select(ids, t["frame_off"].data_ptr(), C.addressof(fo), F, n_rows, t["pt_ids"].data_ptr(), t["n_points"],
                                      t["pt_xyz"].data_ptr(), xys.data_ptr(), cams.data_ptr(), C.addressof(co), C.addressof(cf), cov, C.addressof(vrf),
                                      n_vrf, radius, workspace, workspace_bytes, order.data_ptr(), cnt.data_ptr(), out, st)
    assert select(ids=None) == -1 and b"null" in L.pram_last_error()
    assert select(out=None) == -1
    assert select(workspace_bytes=need - 1) == -1 and b"workspace" in L.pram_last_error()
    assert select(workspace=ws.data_ptr() + 4) == -1 and b"aligned" in L.pram_last_error()
    assert select(vrf=ints([0, 6]), n_vrf=2) == -1 and b"covisible list" in L.pram_last_error()      # frame 6 is no landmark's frame
    assert select(vrf=ints([0, F]), n_vrf=2) == -1 and select(radius=-1.0) == -1 and select(radius=float("nan")) == -1
    assert select(cov=4) == -1 and b"covisibility_frame" in L.pram_last_error()      # the lists are longer than the chain would be
    pt_score = _up(s["pt_obs"].astype(np.int32), dev)

    def sparsify(score=pt_score.data_ptr(), workspace_bytes=need, nkpts=100, radius=20.0):
        return L.pram_compress_sparsify(t["frame_off"].data_ptr(), F, n_rows, cams.data_ptr(), t["pt_xyz"].data_ptr(), score, t["n_points"], radius, nkpts,
                                        ws.data_ptr(), workspace_bytes, lst.data_ptr(), cnt.data_ptr(), st)
    assert sparsify(score=None) == -1 and b"null" in L.pram_last_error()
    assert sparsify(workspace_bytes=24 * n_rows) == -1 and b"workspace" in L.pram_last_error()
    assert sparsify(nkpts=0) == -1 and sparsify(radius=0.0) == -1
    row = torch.zeros(4, device=dev, dtype=torch.int32)
    kp = torch.full((4, 3), -77.0, device=dev, dtype=torch.float64)
    xyz, desc = torch.empty(4, 3, device=dev, dtype=torch.float64), torch.empty(4 * 128 + 4, device=dev)
    sid, ids = torch.empty(4, device=dev, dtype=torch.int32), torch.empty(4, device=dev, dtype=torch.int64)
    err = _up(s["pt_err"], dev)

    def rows(frame=row.data_ptr(), out_desc=desc.data_ptr()):
        return L.pram_compress_rows(frame, row.data_ptr(), 4, F, t["n_points"], cams.data_ptr(), t["pt_ids"].data_ptr(), t["pt_xyz"].data_ptr(),
                                    t["pt_desc"].data_ptr(), t["pt_sid"].data_ptr(), err.data_ptr(), kp.data_ptr(), xyz.data_ptr(), out_desc,
                                    sid.data_ptr(), ids.data_ptr(), st)
    assert rows(frame=None) == -1 and b"null" in L.pram_last_error()
    assert rows(out_desc=desc.data_ptr() + 4) == -1 and b"16-byte" in L.pram_last_error()
    torch.cuda.synchronize()
    assert (order == -77).all() and (cnt == -77).all() and (lst == -77).all() and (kp == -77.0).all()
    # and complete, they succeed
    assert select() == 0 and rows() == 0
    torch.cuda.synchronize()
    want = run["scene"]["results"]["c5"]
    got = order.cpu().numpy()
    assert [int(f) for f in np.argsort(np.where(got < 0, F, got), kind="stable")[:len(want["frames"])]] == want["frames"]
    assert ids.cpu().tolist() == [int(s["pt_ids"][0])] * 4
