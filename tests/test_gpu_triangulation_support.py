"""GPU: stage 2b of the triangulation on the device (pram_tri_adjacency, pram_tri_support, csrc/triangulate.hip) against the numpy
restatement tests/triangulation_support_ref.py: the adjacency and the support counts are integers and compared exactly
(tests/test_triangulation_support_cpu.py asserts the margins that make the counts exact on these scenes, and what each edge of
the star scene is there for), then the public path with ``min_support`` and the C entries' refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import triangulation_ref as TR
from tests import triangulation_support_ref as SR
from tests.test_gpu_triangulation import XYZ_BAR, _same
from tests.test_triangulation_support_cpu import gpu_cases

pytestmark = pytest.mark.gpu

OK, E_ARG = 0, -1      # PRAM_OK, PRAM_E_ARG


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def TG():
    from pram_amd.localization import triangulation
    return triangulation


@pytest.fixture(scope="module")
def cases(TG, dev):
    """name -> (scene, edges, the restatement's support at min_support = 1, the device table), computed once."""
    out = {}
    for name, (s, e) in gpu_cases().items():
        out[name] = (s, e, SR.support(s, e), TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), dev))
    return out


def _adj_equal(got, want):
    return all(got[k].dtype == np.int32 and np.array_equal(got[k], want[k]) for k in ("adj_off", "adj", "row_frame"))


@pytest.mark.parametrize("name", ["star", "tri"])
def test_adjacency_equals_the_restatement(TG, cases, name):
    s, e, r, table = cases[name]
    got = TG.adjacency(table, e)
    assert _adj_equal(got, r["adj"]) and (np.diff(got["adj_off"]) == 0).any() and got["adj_off"][-1] == len(got["adj"])
    if name == "star":
        assert np.diff(got["adj_off"])[s["hub"]] == 200 and np.diff(got["adj_off"])[s["lonely"]] == 0
    rng = np.random.RandomState(6)
    for _ in range(2):      # the order of the edges and of an edge's ends changes nothing
        p = e[rng.permutation(len(e))]
        p = np.where((rng.uniform(size=len(p)) < 0.5)[:, None], p[:, ::-1], p)
        assert _adj_equal(TG.adjacency(table, p), r["adj"])


@pytest.mark.parametrize("n_edges", [0, 1, 255, 256, 257])
def test_adjacency_edge_counts(TG, cases, n_edges):
    """Drawn edges over the planted scene's rows, ends of -1 and of n_rows and loops among them."""
    s, _, _, table = cases["tri"]
    n = int(s["frame_off"][-1])
    e = np.random.RandomState(n_edges).randint(-1, n + 1, size=(n_edges, 2))
    if n_edges >= 255:
        e[7] = (5, 5)
    want = SR.adjacency(n, e, s["frame_off"])
    got = TG.adjacency(table, e)
    assert _adj_equal(got, want) and len(got["adj_off"]) == n + 1 and got["adj_off"][-1] == 2 * SR.valid_edges(n, e).sum()
    assert n_edges < 255 or 0 < SR.valid_edges(n, e).sum() < n_edges


def test_tracks_and_adjacency_past_the_first_chunk_of_block_totals(TG, dev):
    """65 793 rows are 258 blocks of 256 (the adjacency scans one position more): the scan's second level, one workgroup over the
    block totals in chunks of 256, takes a second chunk, and one track and the tail of adj_off have their base there.  Only
    frame_off matters to the two entries; the counts below are the restatement's, asserted so that a change of the inputs cannot
    take the second chunk out of play."""
    n, F = 256 * 256 + 257, 40
    frame_off = np.linspace(0, n, F + 1).astype(int)
    rng = np.random.RandomState(3)
    edges = np.concatenate([rng.randint(0, n, size=(4000, 2)), [[n - 1, n - 2], [-1, 5], [7, n], [9, 9]]])
    kp = np.random.RandomState(4).uniform(0.0, TR.WIDTH, size=(n, 2)).astype(np.float32)
    frames = [{"keypoints": kp[a:b]} for a, b in zip(frame_off[:-1], frame_off[1:])]
    poses = (np.tile([1.0, 0.0, 0.0, 0.0], (F, 1)), np.zeros((F, 3)))
    table = TG.frame_table(frames, [TR.CAMERAS[1]] * F, poses, dev)
    assert table["n_rows"] == n and np.array_equal(table["frame_off_host"], frame_off)
    label = TR.components(n, edges)
    want = {"label": label, **TR.tracks(label, frame_off)}
    want_adj = SR.adjacency(n, edges, frame_off)
    T, E = len(want["trk_label"]), len(want["trk_row"])
    assert int(SR.valid_edges(n, edges).sum()) == 4001 and (T, E) == (3546, 7547) and int(np.diff(want["trk_off"]).max()) == 7
    assert len(want_adj["adj"]) == 8002 and want["trk_label"][want["trk_label"] >= 256 * 256].tolist() == [65791]
    got = TG.build_tracks(table, edges)
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    assert _adj_equal(TG.adjacency(table, edges), want_adj)


@pytest.mark.parametrize("name", ["star", "glued", "tri", "sweep"])
def test_support_equals_the_restatement_and_repeats(TG, cases, name):
    s, e, r, table = cases[name]
    top = int(r["support"].max())
    runs = {ms: TG.support_matches(table, e, min_support=ms) for ms in (1, 2, top + 1)}
    print(f"{name}: {len(e)} edges, {len(r['trace']['edge'])} triples, support up to {top}, {int((r['support'] == 0).sum())} edges without")
    for ms, got in runs.items():
        keep = r["support"] >= ms
        assert got["support"].dtype == np.int32 and np.array_equal(got["support"], r["support"]), (name, ms)
        assert np.array_equal(got["keep"], keep) and np.array_equal(got["edges"], np.where(keep[:, None], e, -1)), (name, ms)
    assert top >= 2 and runs[1]["keep"].any() and not runs[1]["keep"].all() and not runs[top + 1]["keep"].any()
    assert _same(TG.support_matches(table, e, min_support=1), runs[1])
    if name == "star":      # the edges that do not count come back as (-1, -1) whatever they held
        for k in ("none", "past_the_end", "loop"):
            assert runs[1]["edges"][SR.edge_index(s, s["tested"][k])].tolist() == [-1, -1]
    if name == "glued":
        assert runs[1]["support"][e.tolist().index(list(s["bridge"]))] == 0 and runs[1]["keep"].sum() == len(e) - 1


def _map(TG, s, dev, **params):
    return TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev, **params)


@pytest.fixture(scope="module")
def glued_map(TG, dev):
    return _map(TG, SR.glued_scene(), dev, min_support=1)


def test_triangulate_map_recovers_both_glued_points(TG, dev, glued_map):
    s = SR.glued_scene()
    want = SR.run(s, 1)
    m = glued_map
    assert len(m["point_ids"]) == 2 and want["tri"]["accept"].tolist() == [True, True]
    d = np.linalg.norm(m["point3D_xyzs"] - want["tri"]["xyz"], axis=1) / (1.0 + np.linalg.norm(want["tri"]["xyz"], axis=1))
    print(f"glued, min_support = 1: largest |X - X_ref| / (1 + |X_ref|) {d.max():.3e}")
    assert d.max() <= XYZ_BAR
    assert [len(t[0]) for t in m["tracks"].values()] == [4, 4]
    # the support lists: the processed pairs' lengths, -1 exactly where verification dropped the match
    v = TG.verify_matches(TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), dev), s["pairs"], s["matches"])
    assert len(m["support"]) == len(v["keep"]) == len(m["pair_index"])
    for sup, keep in zip(m["support"], v["keep"]):
        assert sup.dtype == np.int32 and sup.shape == keep.shape and np.array_equal(sup == -1, ~keep)
    assert np.array_equal(np.concatenate(m["support"]), want["support"]["support"])
    # without the stage the component yields one point and the result has no support
    one = _map(TG, s, dev)
    assert len(one["point_ids"]) == 1 and "support" not in one and _same(one, _map(TG, s, dev, min_support=0))


def test_support_lists_mark_what_verification_dropped(TG, cases, dev):
    s, e, r, table = cases["tri"]
    m = _map(TG, s, dev, min_support=1)
    v = TG.verify_matches(table, s["pairs"], s["matches"])
    assert [len(x) for x in m["support"]] == [len(k) for k in v["keep"]] and sum(int((~k).sum()) for k in v["keep"]) >= 20
    for sup, keep in zip(m["support"], v["keep"]):
        assert np.array_equal(sup == -1, ~keep)
    assert np.array_equal(np.concatenate(m["support"])[np.concatenate(v["keep"])], r["support"])
    want = SR.run(s, 1)
    ref = TG.map_tables(np.arange(s["n_frames"]), s["frame_off"], want["tracks"], want["tri"])
    assert np.array_equal(m["point_ids"], ref["point_ids"]) and _same(m["tracks"], ref["tracks"])
    assert np.abs(m["point3D_xyzs"] - ref["point3D_xyzs"]).max() <= XYZ_BAR * (1 + np.abs(ref["point3D_xyzs"]).max())


def test_default_is_the_stages_run_by_hand(TG, cases, dev):
    s, _, _, table = cases["tri"]
    m = _map(TG, s, dev)
    v = TG.verify_matches(table, s["pairs"], s["matches"])
    edges = np.concatenate([s["frame_off"][s["pairs"][i]] + k for i, k in zip(v["pair_index"].tolist(), v["kept"])])
    trk = TG.build_tracks(table, edges)
    want = TG.map_tables(np.arange(s["n_frames"]), s["frame_off"], trk, TG.triangulate_tracks(table, trk))
    assert set(m) == set(want) | {"pair_index", "inlier_ratio"}
    assert all(_same(m[k], want[k]) for k in want)


def test_glued_map_into_a_reference_store(TG, dev, glued_map):
    from pram_amd.localization import labelling as LB
    from pram_amd.localization import mapbuild as MB
    from pram_amd.localization.candidates import ReferenceStore
    from tests import pose_ref as PR
    s, m = SR.glued_scene(), glued_map
    xyz = dict(zip(m["point_ids"].tolist(), m["point3D_xyzs"]))
    lab = LB.label_points(m["tracks"], xyz, 2, dev, min_obs=2)
    landmarks, sids = LB.landmarks_from_labels(lab["id"], lab["label"])
    assert sorted(sids) == [1, 2]
    rng = np.random.RandomState(9)
    frames = []
    for f in range(s["n_frames"]):
        kp = s["frames"][f]["keypoints"]
        d = rng.normal(size=(len(kp), 128)).astype(np.float32)
        pid = m["frames"][f]["point3D_ids"]
        fx, fy, cx, cy = PR.unify(int(s["cam_model"][f]), s["cam_params"][f])[:4]
        frames.append({"keypoints": np.concatenate([kp, np.ones((len(kp), 1), dtype=np.float32)], 1), "descriptors": d / np.linalg.norm(d, axis=1, keepdims=True),
                       "xyzs": m["frames"][f]["xyzs"], "point3D_ids": pid, "keypoint_segs": np.array([sids.get(int(p), 0) for p in pid], dtype=np.int32),
                       "width": TR.WIDTH, "height": TR.HEIGHT, "qvec": s["qvec"][f], "tvec": s["tvec"][f], "intrinsics": (fx, fy, cx, cy)})
    out = MB.build_store_inputs(frames, m["tracks"], landmarks, xyz, dev, min_obs=2, n_vrf=3)
    store = ReferenceStore(frames, point3D_sids=sids, **{k: out[k] for k in MB.STORE_KEYS})
    assert store.pt_ids.tolist() == [1, 2] and np.array_equal(store._point_values()["pt_xyz"], m["point3D_xyzs"])
    assert (store.point3D_ids >= 1).sum() == 8


# ---------------------------------------------------------------- the C entries
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _adjacency_args(hip_lib, s, e, dev, fill=-7):
    n, F, m = int(s["frame_off"][-1]), s["n_frames"], len(e)
    t = {"edges": torch.from_numpy(np.ascontiguousarray(e, dtype=np.int32)).to(dev), "frame_off": torch.from_numpy(s["frame_off"]).to(dev),
         "ws": torch.empty(int(hip_lib.pram_tri_adjacency_workspace_bytes(n, m)), device=dev, dtype=torch.uint8),
         "adj_off": torch.full((n + 1 + 8,), fill, device=dev, dtype=torch.int32), "adj": torch.full((2 * m + 8,), fill, device=dev, dtype=torch.int32),
         "row_frame": torch.full((n + 8,), fill, device=dev, dtype=torch.int32)}
    return t, n, F, m


def test_c_entries_write_their_ranges_only_and_refuse(hip_lib, cases, dev):
    from pram_amd import _lib
    L = hip_lib
    s, e, r, table = cases["star"]
    t, n, F, m = _adjacency_args(L, s, e, dev)
    adj_call = lambda **o: L.pram_tri_adjacency(o.get("edges", _p(t["edges"])), o.get("m", m), _p(t["frame_off"]), o.get("F", F), o.get("n", n), o.get("ws", _p(t["ws"])),
                                                o.get("ws_bytes", t["ws"].numel()), _p(t["adj_off"]), o.get("adj", _p(t["adj"])), _p(t["row_frame"]), None)
    assert adj_call() == OK
    n_adj = int(r["adj"]["adj_off"][-1])
    assert n_adj < 2 * m      # five edges do not count: the tail of adj is not written
    assert np.array_equal(t["adj_off"][:n + 1].cpu().numpy(), r["adj"]["adj_off"]) and (t["adj_off"][n + 1:] == -7).all()
    assert np.array_equal(t["adj"][:n_adj].cpu().numpy(), r["adj"]["adj"]) and (t["adj"][n_adj:] == -7).all()
    assert np.array_equal(t["row_frame"][:n].cpu().numpy(), r["adj"]["row_frame"]) and (t["row_frame"][n:] == -7).all()
    sup = torch.full((m + 8,), -7, device=dev, dtype=torch.int32)
    out = torch.full((m + 8, 2), -7, device=dev, dtype=torch.int32)
    one = torch.zeros(8, device=dev, dtype=torch.float64)
    sup_call = lambda **o: L.pram_tri_support(o.get("norm", _p(table["norm05"])), _p(table["keypoints"]), _p(table["frames"]), _p(table["cam_model"]), _p(table["cam_params"]),
                                              _p(t["edges"]), o.get("m", m), _p(t["adj_off"]), _p(t["adj"]), _p(t["row_frame"]), F, o.get("n", n),
                                              ctypes.c_double(o.get("angle", float(np.deg2rad(1.5)))), ctypes.c_double(o.get("err", 4.0)), o.get("ms", 1),
                                              o.get("sup", _p(sup)), _p(out), None)
    assert sup_call() == OK
    assert np.array_equal(sup[:m].cpu().numpy(), r["support"]) and (sup[m:] == -7).all()
    assert np.array_equal(out[:m].cpu().numpy(), r["edges"]) and (out[m:] == -7).all()
    # min_support = 0 keeps every edge as it came, the ones that do not count included
    assert sup_call(ms=0) == OK and np.array_equal(out[:m].cpu().numpy(), e.astype(np.int32))
    # no edges, no rows: valid, and only adj_off / row_frame are written
    for o in ({"m": 0}, {"m": 0, "n": 0, "F": 0}):
        t["adj_off"].fill_(-7); t["adj"].fill_(-7)
        assert adj_call(**o) == OK and sup_call(**{k: v for k, v in o.items() if k != "F"}) == OK
        rows = o.get("n", n)
        assert not t["adj_off"][:rows + 1].any() and (t["adj_off"][rows + 1:] == -7).all() and (t["adj"] == -7).all()
    # ---- refusals
    null, odd = ctypes.c_void_p(0), ctypes.c_void_p(t["ws"].data_ptr() + 1)
    assert L.pram_tri_adjacency_workspace_bytes(-1, 1) == 0 and L.pram_tri_adjacency_workspace_bytes(2 ** 30 + 1, 1) == 0
    assert L.pram_tri_adjacency_workspace_bytes(1, -1) == 0 and L.pram_tri_adjacency_workspace_bytes(1, 2 ** 30) == 0
    assert L.pram_tri_adjacency_workspace_bytes(0, 0) > 0
    for o in ({"edges": null}, {"adj": null}, {"ws": null}, {"edges": odd}, {"ws": odd}, {"m": -1}, {"n": -1}, {"F": -1}, {"n": 2 ** 30 + 1}, {"m": 2 ** 30},
              {"F": 0}, {"ws_bytes": t["ws"].numel() - 1}, {"ws_bytes": int(L.pram_tri_adjacency_workspace_bytes(n, m)) - 1}):
        assert adj_call(**o) == E_ARG, o
    for o in ({"norm": null}, {"sup": null}, {"norm": ctypes.c_void_p(one.data_ptr() + 4)}, {"sup": odd}, {"m": -1}, {"n": -1}, {"n": 2 ** 30 + 1}, {"ms": -1},
              {"err": 0.0}, {"err": -1.0}, {"err": float("nan")}, {"angle": -0.1}, {"angle": float("nan")}):
        assert sup_call(**o) == E_ARG, o
    assert b"pram_tri_support" in L.pram_last_error()
    from pram_amd import ops
    with pytest.raises(_lib.PramHipError):
        ops.tri_adjacency(t["edges"], m, t["frame_off"], F, n, workspace=t["ws"][:-1])


def test_a_table_that_is_not_ours_leads_nowhere(TG, cases, dev):
    """Offsets past the table, below zero and descending, neighbours and frames outside their ranges: every read stays inside
    (the offsets are clamped, such a neighbour is skipped), and the edges whose lists are untouched keep their counts."""
    from pram_amd import ops
    s, e, r, table = cases["glued"]
    n, m = int(s["frame_off"][-1]), len(e)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    run = lambda a: ops.tri_support(table["norm05"], table["keypoints"], table["frames"], table["cam_model"], table["cam_params"], up(e), m,
                                    up(a["adj_off"]), up(a["adj"]), up(a["row_frame"]), s["n_frames"], n)["support"][:m].cpu().numpy()
    assert np.array_equal(run(r["adj"]), r["support"])
    adj = {k: v.copy() for k, v in r["adj"].items()}
    adj["adj"][::3] = np.array([-5, n, 2 ** 30])[np.arange(len(adj["adj"][::3])) % 3]      # such a neighbour is never dereferenced
    got = run(adj)
    assert (got >= 0).all() and (got <= len(adj["adj"])).all()
    for off in (np.full(n + 1, 2 ** 30), np.full(n + 1, -4), r["adj"]["adj_off"][::-1].copy()):      # every list is empty
        assert not run({**r["adj"], "adj_off": off}).any()
    rf = r["adj"]["row_frame"].copy()
    u = int(e[0, 0])
    rf[u] = s["n_frames"]
    got = run({**r["adj"], "row_frame": rf})
    touched = (e == u).any(1) | np.isin(np.arange(m), r["trace"]["edge"][r["trace"]["rows"][:, 2] == u])
    assert not got[(e == u).any(1)].any() and np.array_equal(got[~touched], r["support"][~touched])
