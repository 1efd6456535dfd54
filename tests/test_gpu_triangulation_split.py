"""GPU: the triangulation's further rounds on the device (pram_tri_split of csrc/triangulate.hip, ``split_rounds`` of
triangulate_map) against the numpy restatement tests/triangulation_split_ref.py: states, filtered edges and counts are bytes and
integers and compared exactly, and so are the labels, tables and discrete results of every round
(tests/test_triangulation_split_cpu.py asserts the margins that make them exact on these scenes); positions and errors within the
bars of tests/test_gpu_triangulation.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import triangulation_ref as TR
from tests import triangulation_split_ref as PL
from tests import triangulation_support_ref as SR

pytestmark = pytest.mark.gpu

OK, E_ARG = 0, -1      # PRAM_OK, PRAM_E_ARG
XYZ_BAR = 1e-14        # tests/test_gpu_triangulation.py's, restated: on |X - X_ref| / (1 + |X_ref|) and on the errors in pixels


def test_the_bar_is_the_one_of_the_triangulation_test():
    from tests import test_gpu_triangulation as T
    assert XYZ_BAR == T.XYZ_BAR


def _same(a, b) -> bool:
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def TG():
    from pram_amd.localization import triangulation
    return triangulation


def _table(TG, s, dev):
    return TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), dev)


def _map(TG, s, dev, **params):
    return TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev, **params)


# ---------------------------------------------------------------- the entry against the restatement
def _check_split(TG, table, n, trk, tri, edges, state=None):
    want = PL.split(n, trk, tri, edges, state)
    got = TG.split_edges(table, edges, trk, tri, state)
    assert got["state"].dtype == np.uint8 and got["state"].shape == (n,) and np.array_equal(got["state"], want["state"])
    assert got["edges"].dtype == np.int32 and np.array_equal(got["edges"], want["edges"].reshape(-1, 2)) and got["n_live"] == want["n_live"]
    assert _same(TG.split_edges(table, edges, trk, tri, state), got)      # again: the same bytes
    return want


def _drawn_results(rng, trk):
    """accept and entry_keep drawn over a table: accepted and refused tracks, kept and dropped entries in each."""
    T, E = len(trk["trk_off"]) - 1, len(trk["trk_row"])
    return {"accept": rng.uniform(size=T) < 0.7, "entry_keep": rng.uniform(size=E) < 0.5}


def _drawn_edges(rng, n, m):
    """m edges over [-1, n]: ends of -1 and of n_rows, loops and duplicates among them from 255 on."""
    e = rng.randint(-1, n + 1, size=(m, 2))
    if m >= 255:
        e[7], e[9], e[11], e[12] = (5, 5), e[8], e[10][::-1], (-1, -1)
    return e


def test_ring_tracks_of_2_3_63_64_65_entries(TG, dev):
    s = TR.ring_scene()
    r = TR.run(s)
    n, trk = int(s["frame_off"][-1]), r["tracks"]
    assert sorted(np.diff(trk["trk_off"]).tolist()) == [2, 3, 17, 63, 64, 65]
    table = _table(TG, s, dev)
    rng = np.random.RandomState(1)
    edges = np.concatenate([r["verify"]["edges"], _drawn_edges(rng, n, 300)])
    for accept in ([True] * 6, [False] * 6, [True, False] * 3, [False, True] * 3):
        tri = {"accept": np.array(accept), "entry_keep": rng.uniform(size=len(trk["trk_row"])) < 0.4}
        w = _check_split(TG, table, n, trk, tri, edges)
        assert 0 < w["n_live"] < len(edges) or not any(accept)
    tri = {"accept": np.ones(6, dtype=bool), "entry_keep": np.zeros(len(trk["trk_row"]), dtype=bool)}      # everything FREE: every valid edge stays
    w = _check_split(TG, table, n, trk, tri, edges)
    assert (w["state"] == PL.FREE).all() and w["n_live"] >= len(r["verify"]["edges"])
    # the round's own results, and a second round on the state of the first
    w = _check_split(TG, table, n, trk, r["tri"], edges)
    assert (w["state"] == PL.TAKEN).sum() == int(r["tri"]["entry_keep"].sum())
    _check_split(TG, table, n, trk, {"accept": np.array([True, False] * 3), "entry_keep": np.zeros(len(trk["trk_row"]), dtype=bool)}, edges, w["state"])


@pytest.mark.parametrize("n_entries", [255, 256, 257])
def test_entry_counts_around_a_workgroup(TG, dev, n_entries):
    """Tracks of 2 to 9 entries over the sweep scene's rows, cut to the entry count: the last workgroup is full, one short, one over."""
    s = SR.sweep_scene(0.05, PL.SWEEP_SEED)
    n = int(s["frame_off"][-1])
    rng = np.random.RandomState(n_entries)
    sizes = []
    while sum(sizes) < n_entries:
        sizes.append(min(int(rng.randint(2, 10)), n_entries - sum(sizes)))
    rows = rng.permutation(n)[:n_entries]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    trk = {"trk_off": off, "trk_row": np.concatenate([np.sort(rows[a:b]) for a, b in zip(off[:-1], off[1:])]).astype(np.int32)}
    assert len(trk["trk_row"]) == n_entries
    tri = _drawn_results(rng, trk)
    w = _check_split(TG, _table(TG, s, dev), n, trk, tri, _drawn_edges(rng, n, 2000))
    assert {PL.FREE, PL.TAKEN, PL.DEAD} == set(w["state"].tolist()) and w["n_live"] > 0


@pytest.mark.parametrize("n_edges", [0, 1, 255, 256, 257])
def test_edge_counts_and_one_track(TG, dev, n_edges):
    """One track that holds every second row, half of its entries kept; the edges drawn, and with one edge a live one."""
    s = SR.sweep_scene(0.05, PL.SWEEP_SEED)
    n = int(s["frame_off"][-1])
    rng = np.random.RandomState(n_edges)
    rows = np.arange(0, n, 2, dtype=np.int32)
    trk = {"trk_off": np.array([0, len(rows)], dtype=np.int32), "trk_row": rows}
    tri = {"accept": np.array([True]), "entry_keep": np.arange(len(rows)) % 2 == 0}
    edges = np.array([[2, 6]]) if n_edges == 1 else np.where(rng.uniform(size=(n_edges, 1)) < 0.5, 2 + 4 * rng.randint(0, n // 4 - 1, size=(n_edges, 2)), _drawn_edges(rng, n, n_edges))
    w = _check_split(TG, _table(TG, s, dev), n, trk, tri, edges)
    assert (w["state"][2::4] == PL.FREE).all() and (w["state"][0::4] == PL.TAKEN).all() and (w["state"][1::2] == PL.DEAD).all()
    assert (w["n_live"] > 0) == (n_edges > 0) and (n_edges < 255 or w["n_live"] < n_edges)
    if n_edges == 1:
        _check_split(TG, _table(TG, s, dev), n, {"trk_off": np.zeros(1, dtype=np.int32), "trk_row": np.zeros(0, dtype=np.int32)},
                     {"accept": np.zeros(0, dtype=bool), "entry_keep": np.zeros(0, dtype=bool)}, edges)      # no track: every row DEAD, no edge


# ---------------------------------------------------------------- triangulate_map, round by round
@pytest.fixture(scope="module")
def maps(TG, dev):
    """name -> (scene, the restatement's run, the device's map), computed once."""
    out = {}
    for name in ("glued", "chain", "dead", "lone1", "lone2", "sweep05", "sweep10"):
        s, ms, R, r = PL.gpu_run(name)
        out[name] = (s, ms, R, r, _map(TG, s, dev, min_support=ms, split_rounds=R))
    return out


@pytest.mark.parametrize("name", ["glued", "chain", "dead", "lone1", "lone2", "sweep05", "sweep10"])
def test_every_round_equals_the_restatement(TG, dev, maps, name):
    s, ms, R, r, m = maps[name]
    n, table = int(s["frame_off"][-1]), _table(TG, s, dev)
    state, worst = None, 0.0
    for k, x in enumerate(r["rounds"]):
        if k:      # the step into round k: state, edges and the count
            prev = r["rounds"][k - 1]
            got = TG.split_edges(table, r["edges"], prev["tracks"], prev["tri"], state)
            assert np.array_equal(got["state"], x["state"]) and np.array_equal(got["edges"], x["edges"]) and got["n_live"] == x["n_live"], (name, k)
            state = got["state"]
        if x["tracks"] is None:
            continue
        trk = TG.build_tracks(table, r["edges"] if k == 0 else x["edges"])
        assert np.array_equal(trk["label"], x["label"]), (name, k)
        for key in ("trk_off", "trk_label", "trk_row", "trk_frame", "trk_kpt"):
            assert trk[key].dtype == np.int32 and np.array_equal(trk[key], x["tracks"][key]), (name, k, key)
        got, want = TG.triangulate_tracks(table, trk), x["tri"]
        for key in ("accept", "kept", "best", "entry_keep"):
            assert np.array_equal(got[key], want[key]), (name, k, key)
        assert np.array_equal(got["entry_error"] >= 0, want["entry_error"] >= 0)
        ok = want["best"] >= 0
        dx = np.linalg.norm(got["xyz"][ok] - want["xyz"][ok], axis=1) / (1.0 + np.linalg.norm(want["xyz"][ok], axis=1))
        de, dee = np.abs(got["error"] - want["error"]), np.abs(got["entry_error"] - want["entry_error"])
        worst = max(worst, float(dx.max(initial=0.0)), float(de.max(initial=0.0)), float(dee.max(initial=0.0)))
        assert dx.max(initial=0.0) <= XYZ_BAR and de.max(initial=0.0) <= XYZ_BAR and dee.max(initial=0.0) <= XYZ_BAR, (name, k)
    # ---- and the map is those rounds, one after the other
    xyz, rnd = PL.points(r)
    print(f"{name}: {len(r['rounds'])} rounds, {len(xyz)} points, largest deviation of a position or an error {worst:.3e}")
    want = TG.split_tables(np.arange(s["n_frames"]), s["frame_off"], [(x["tracks"], x["tri"]) for x in PL.complete(r)])
    assert np.array_equal(m["point_ids"], want["point_ids"]) and np.array_equal(m["point_round"], rnd) and m["point_round"].dtype == np.int32
    assert _same(m["tracks"], want["tracks"]) and _same([f["point3D_ids"] for f in m["frames"]], [f["point3D_ids"] for f in want["frames"]])
    assert np.abs(m["point3D_xyzs"] - xyz).max() <= XYZ_BAR * (1 + np.abs(xyz).max()) and np.abs(m["track_error"] - want["track_error"]).max() <= XYZ_BAR
    begun = r["rounds"][1:]
    assert m["split"]["live_edges"].tolist() == [x["n_live"] for x in begun]
    assert m["split"]["tracks"].tolist() == [0 if x["tracks"] is None else len(x["tracks"]["trk_label"]) for x in begun]
    assert m["split"]["points"].tolist() == [0 if x["tracks"] is None else int(x["tri"]["accept"].sum()) for x in begun]
    assert ("support" in m) == (ms > 0)


def test_what_the_scenes_are_for(maps):
    s, _, _, _, m = maps["glued"]
    assert m["point_round"].tolist() == [0, 1] and [len(t[0]) for t in m["tracks"].values()] == [4, 4]
    assert m["point_round"].tolist() == maps["dead"][4]["point_round"].tolist() and maps["chain"][4]["point_round"].tolist() == [0, 1, 1]
    far = maps["dead"][0]["point_rows"][PL.FAR]
    assert (np.concatenate([f["point3D_ids"] for f in maps["dead"][4]["frames"]])[far] == -1).all()
    for name in ("lone1", "lone2"):
        assert len(maps[name][4]["point_ids"]) == 1 and maps[name][4]["split"]["live_edges"].tolist() == [0]
    for name, more in (("sweep05", 15), ("sweep10", 35)):
        s, _, R, _, m = maps[name]
        found = [len(PL.distinct_found(s, m["point3D_xyzs"][m["point_round"] <= k])) for k in range(R + 1)]
        print(f"{name}: distinct planted points found after each round {found}")
        assert found[-1] >= found[0] + more and all(b >= a for a, b in zip(found[:-1], found[1:]))


def test_a_leftover_of_one_frame_joined_by_an_edge_is_refused_and_dead(TG, dev, maps):
    """The two leftover rows of lone2 lie in one frame; with an edge between them (no match can be one, so the stages are run by
    hand) round 1 has one track that stage 4 cannot accept, and round 2 finds its rows DEAD and no edge."""
    s, _, _, r, _ = maps["lone2"]
    lone = [s["point_rows"][1][0], s["point_rows"][2][0]]
    edges = np.concatenate([r["edges"], [lone]])
    want = PL.rounds(s, edges, 3)
    assert [x["n_live"] for x in want[1:]] == [1, 0] and want[1]["tri"]["accept"].tolist() == [False]
    table = _table(TG, s, dev)
    trk = TG.build_tracks(table, edges)
    tri = TG.triangulate_tracks(table, trk)
    one = TG.split_edges(table, edges, trk, tri)
    assert np.array_equal(one["state"], want[1]["state"]) and np.array_equal(one["edges"], want[1]["edges"]) and one["n_live"] == 1
    trk = TG.build_tracks(table, one["edges"])
    tri = TG.triangulate_tracks(table, trk)
    assert trk["trk_row"].tolist() == sorted(lone) and len(set(trk["trk_frame"].tolist())) == 1
    assert tri["accept"].tolist() == [False] and tri["best"].tolist() == [-1] and not tri["entry_keep"].any()
    two = TG.split_edges(table, edges, trk, tri, one["state"])
    assert np.array_equal(two["state"], want[2]["state"]) and (two["state"][lone] == PL.DEAD).all() and two["n_live"] == 0 and (two["edges"] == -1).all()


@pytest.mark.parametrize("name", ["glued", "chain", "sweep05"])
def test_round_0_is_the_run_without_rounds_bit_for_bit(TG, dev, maps, name):
    s, ms, R, _, m = maps[name]
    base = _map(TG, s, dev, min_support=ms)
    assert "point_round" not in base and "split" not in base and _same(base, _map(TG, s, dev, min_support=ms, split_rounds=0))
    P0 = len(base["point_ids"])
    assert 0 < P0 < len(m["point_ids"]) and (m["point_round"][:P0] == 0).all() and (m["point_round"][P0:] > 0).all()
    for k in ("point_ids", "point3D_xyzs", "track_error"):
        assert _same(m[k][:P0], base[k]), k
    assert _same({p: m["tracks"][p] for p in base["tracks"]}, base["tracks"]) and _same(m["pair_index"], base["pair_index"])
    for fm, fb in zip(m["frames"], base["frames"]):
        was = fb["point3D_ids"] >= 1
        assert _same(fm["point3D_ids"][was], fb["point3D_ids"][was]) and _same(fm["xyzs"][was], fb["xyzs"][was])
        assert ((fm["point3D_ids"][~was] == -1) | (fm["point3D_ids"][~was] > P0)).all()
    if ms:
        assert _same(m["support"], base["support"])


@pytest.mark.parametrize("name", ["chain", "sweep05"])
def test_the_order_of_pairs_and_matches_changes_nothing(TG, dev, maps, name):
    s, ms, R, r, m = maps[name]
    rng = np.random.RandomState(8)
    order = rng.permutation(r["pair_index"])
    shuffled = [s["matches"][i][rng.permutation(len(s["matches"][i]))] for i in order.tolist()]
    again = TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"][order], shuffled, dev, min_support=ms, split_rounds=R)
    for k in ("point_ids", "point3D_xyzs", "track_error", "tracks", "frames", "point_round", "split"):
        assert _same(again[k], m[k]), k
    assert _same(_map(TG, s, dev, min_support=ms, split_rounds=R), m)      # and a second run gives the same bytes


def test_glued_map_with_a_round_into_a_reference_store(TG, dev, maps):
    from pram_amd.localization import labelling as LB
    from pram_amd.localization import mapbuild as MB
    from pram_amd.localization.candidates import ReferenceStore
    from tests import pose_ref as PR
    s, _, _, _, m = maps["glued"]
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


# ---------------------------------------------------------------- the C entry
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _args(dev, n, trk, tri, edges, fill=7):
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    m = len(edges)
    return {"trk_off": up(trk["trk_off"], np.int32), "trk_row": up(trk["trk_row"], np.int32), "accept": up(tri["accept"], np.int32),
            "entry_keep": up(tri["entry_keep"], np.uint8), "edges": up(np.asarray(edges).reshape(-1, 2), np.int32),
            "state": torch.full((n + 8,), fill, device=dev, dtype=torch.uint8), "out": torch.full((m + 8, 2), -7, device=dev, dtype=torch.int32),
            "n_live": torch.full((9,), -7, device=dev, dtype=torch.int32)}


def test_c_entry_writes_its_ranges_only_and_refuses(hip_lib, dev):
    L = hip_lib
    s, _, _, r = PL.gpu_run("chain")
    n, trk, tri, edges = int(s["frame_off"][-1]), r["tracks"], r["tri"], r["edges"]
    T, E, m = len(trk["trk_label"]), len(trk["trk_row"]), len(edges)
    t = _args(dev, n, trk, tri, edges)
    call = lambda **o: L.pram_tri_split(o.get("trk_off", _p(t["trk_off"])), _p(t["trk_row"]), o.get("T", T), o.get("E", E), o.get("accept", _p(t["accept"])),
                                        _p(t["entry_keep"]), o.get("edges", _p(t["edges"])), o.get("m", m), o.get("n", n), o.get("first", 1),
                                        o.get("state", _p(t["state"])), o.get("out", _p(t["out"])), o.get("n_live", _p(t["n_live"])), None)
    want = PL.split(n, trk, tri, edges)
    assert call() == OK
    assert np.array_equal(t["state"][:n].cpu().numpy(), want["state"]) and (t["state"][n:] == 7).all()
    assert np.array_equal(t["out"][:m].cpu().numpy(), want["edges"]) and (t["out"][m:] == -7).all()
    assert t["n_live"][0].item() == want["n_live"] == 12 and (t["n_live"][1:] == -7).all()
    # first = 0 marks onto the state as it is: the rows of no track keep the caller's byte
    t["state"].fill_(7)
    assert call(first=0) == OK
    got = t["state"][:n].cpu().numpy()
    touched = np.isin(np.arange(n), trk["trk_row"])
    assert np.array_equal(got[touched], want["state"][touched]) and (got[~touched] == 7).all() and (t["state"][n:] == 7).all()
    # no tracks, no edges, no rows: valid; the count is written, edges_out is not
    for o, live in (({"T": 0, "E": 0}, 0), ({"m": 0}, 0), ({"n": 0}, 0), ({"T": 0, "E": 0, "m": 0, "n": 0}, 0)):
        t["state"].fill_(7); t["out"].fill_(-7); t["n_live"].fill_(-7)
        assert call(**o) == OK and t["n_live"][0].item() == live and (t["n_live"][1:] == -7).all(), o
        rows, em = o.get("n", n), o.get("m", m)
        assert (t["state"][rows:] == 7).all() and (t["out"][em:] == -7).all() and (t["out"][:em] == -1).all()
        assert not (t["state"][:rows] == 7).any() and (o.get("T", T) or (t["state"][:rows] == PL.DEAD).all())
    # ---- refusals
    null, odd = ctypes.c_void_p(0), ctypes.c_void_p(t["trk_off"].data_ptr() + 1)
    for o in ({"trk_off": null}, {"accept": null}, {"edges": null}, {"state": null}, {"out": null}, {"n_live": null}, {"trk_off": odd}, {"edges": odd},
              {"out": odd}, {"n_live": odd}, {"T": -1}, {"E": -1}, {"m": -1}, {"n": -1}, {"n": 2 ** 30 + 1}, {"m": 2 ** 30}, {"E": 2 ** 30 + 1},
              {"first": 2}, {"first": -1}):
        assert call(**o) == E_ARG, o
    assert b"pram_tri_split" in L.pram_last_error()


def test_a_table_that_is_not_ours_leads_nowhere(TG, dev):
    """Offsets past the table, below zero and descending, rows outside [0, n_rows): every read and write stays inside, the bytes
    beyond the state and the edges beyond n_edges keep what they held, and the state holds nothing but the three values."""
    from pram_amd import ops
    s, _, _, r = PL.gpu_run("sweep05")
    n, trk, tri, edges = int(s["frame_off"][-1]), r["tracks"], r["tri"], r["edges"]
    T, E, m = len(trk["trk_label"]), len(trk["trk_row"]), len(edges)
    want = PL.split(n, trk, tri, edges)
    rows = trk["trk_row"].copy()
    rows[::3] = np.array([-5, n, 2 ** 30])[np.arange(len(rows[::3])) % 3]
    cases = [({**trk, "trk_row": rows}, "rows"), ({**trk, "trk_off": np.full(T + 1, 2 ** 30, dtype=np.int32)}, "past"),
             ({**trk, "trk_off": np.full(T + 1, -4, dtype=np.int32)}, "below"), ({**trk, "trk_off": trk["trk_off"][::-1].copy()}, "descending")]
    for bad, what in cases:
        t = _args(dev, n, bad, tri, edges)
        out = ops.tri_split(t["trk_off"], t["trk_row"], T, E, t["accept"], t["entry_keep"], t["edges"], m, n)
        torch.cuda.synchronize()
        st, eo = out["state"][:n].cpu().numpy(), out["edges"][:m].cpu().numpy()
        assert set(st.tolist()) <= {PL.FREE, PL.TAKEN, PL.DEAD} and int(out["n_live"].item()) == int((eo >= 0).all(1).sum()), what
        assert ((eo == -1).all(1) | (eo == np.asarray(edges)).all(1)).all(), what
        if what == "rows":      # the entries that name a row of the table are marked as before, nothing else is
            ok = np.ones(E, dtype=bool)
            ok[::3] = False
            hit = np.isin(np.arange(n), trk["trk_row"][ok])
            assert np.array_equal(st[hit], want["state"][hit]) and (st[~hit] == PL.DEAD).all()
        elif what != "descending":      # every track is empty
            assert (st == PL.DEAD).all() and int(out["n_live"].item()) == 0
