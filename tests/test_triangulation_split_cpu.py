"""CPU: the triangulation's further rounds, ``split_rounds`` (tests/triangulation_split_ref.py): marking and filtering against a
version written with sets, the glued, chain, dead and lone scenes, what the rounds recover on the simulation, the margins that
make the device's discrete results exact on every track of every round the GPU test runs, and the host side of
pram_amd.localization.triangulation with ops replaced by the restatement."""
import numpy as np
import pytest
import torch

from tests import triangulation_ref as TR
from tests import triangulation_split_ref as PL
from tests import triangulation_support_ref as SR
from tests.test_triangulation_cpu import _bound
from tests.test_triangulation_support_cpu import StubOps, _map

MIN_ANGLE = float(np.deg2rad(TR.DEFAULTS["min_tri_angle"]))
MAX_REPROJ = TR.DEFAULTS["max_reproj_error"]


def test_symbol_declared_exported_and_wrapped(hip_lib):
    from pram_amd import _lib, ops
    # the entry's declaration, types and export and header == ops for PRAM_TRI_ROW_*: tests/test_abi_contract_cpu.py
    assert "pram_tri_split" in _lib.exported_symbols()
    assert (PL.FREE, PL.TAKEN, PL.DEAD) == (ops.TRI_ROW_FREE, ops.TRI_ROW_TAKEN, ops.TRI_ROW_DEAD)
    assert callable(ops.tri_split)


# ---------------------------------------------------------------- marking and filtering, with sets
def set_split(n_rows: int, trk: dict, tri: dict, edges, state) -> dict:
    """The rows as three sets instead of a byte each."""
    free = set() if state is None else set(np.nonzero(state == PL.FREE)[0].tolist())
    taken = set() if state is None else set(np.nonzero(state == PL.TAKEN)[0].tolist())
    for t, (a, b) in enumerate(zip(trk["trk_off"][:-1], trk["trk_off"][1:])):
        rows = set(trk["trk_row"][a:b].tolist())
        kept = set(trk["trk_row"][a:b][tri["entry_keep"][a:b]].tolist()) if tri["accept"][t] else set()
        free = (free - rows) | ((rows - kept) if tri["accept"][t] else set())
        taken = (taken - rows) | kept
    live = [i for i, (u, v) in enumerate(np.asarray(edges).reshape(-1, 2).tolist()) if u in free and v in free]
    return {"free": free, "taken": taken, "live": live}


@pytest.mark.parametrize("name", ["sweep10", "sweep05", "chain", "dead"])
def test_marking_and_filtering_equal_the_version_with_sets(name):
    s, ms, R, r = PL.gpu_run(name)
    n = int(s["frame_off"][-1])
    rng = np.random.RandomState(2)
    extra = np.concatenate([rng.randint(-2, n + 2, size=(40, 2)), [[-1, -1], [n, 0], [0, n], [3, 3]]])
    edges = np.concatenate([np.asarray(r["edges"], dtype=np.int64), extra, np.asarray(r["edges"][:5], dtype=np.int64)[:, ::-1]])      # out of range, loops, duplicates
    state = None
    for k, x in enumerate(PL.complete(r)):
        got = PL.split(n, x["tracks"], x["tri"], edges, state)
        want = set_split(n, x["tracks"], x["tri"], edges, state)
        assert set(np.nonzero(got["state"] == PL.FREE)[0].tolist()) == want["free"], (name, k)
        assert set(np.nonzero(got["state"] == PL.TAKEN)[0].tolist()) == want["taken"], (name, k)
        assert np.nonzero((got["edges"] >= 0).all(1))[0].tolist() == want["live"] and got["n_live"] == len(want["live"]), (name, k)
        assert np.array_equal(got["edges"][want["live"]], edges[want["live"]]) and (np.delete(got["edges"], want["live"], 0) == -1).all()
        if state is not None:      # a row only ever goes FREE -> TAKEN or FREE -> DEAD
            changed = np.nonzero(state != got["state"])[0]
            assert (state[changed] == PL.FREE).all() and (got["state"][changed] != PL.FREE).all(), (name, k)
        state = got["state"]
    assert k >= 1


# ---------------------------------------------------------------- the planted scenes
def test_glued_scene_one_point_then_two():
    s = SR.glued_scene()
    r0, r1, sup = PL.run(s, 0, 0), PL.run(s, 0, 1), PL.run(s, 1, 0)
    assert len(r0["rounds"]) == 1 and len(PL.points(r0)[0]) == 1
    xyz, rnd = PL.points(r1)
    assert rnd.tolist() == [0, 1] and np.array_equal(xyz[0], PL.points(r0)[0][0])
    one = r1["rounds"][1]
    assert one["n_live"] == 6 and np.diff(one["tracks"]["trk_off"]).tolist() == [4] and one["tri"]["kept"].tolist() == [4]
    assert np.array_equal(xyz[1], sup["tri"]["xyz"][1]) and sup["tri"]["accept"].tolist() == [True, True]      # the point min_support = 1 recovers
    d = [float(np.linalg.norm(xyz[k] - s["xyz"][k])) for k in (0, 1)]
    print(f"glued: |X - X*| = {d[0]:.4f} (round 0), {d[1]:.4f} (round 1)")
    state = one["state"]
    assert (state == PL.TAKEN).sum() == 4 and (state == PL.FREE).sum() == 4 and not (state == PL.DEAD).any()


def test_chain_scene_three_points_after_one_further_round():
    """Round 0 keeps the middle point B, which frees A and C from each other: both come in round 1, and round 2 finds no edge."""
    s = PL.chain_scene()
    r = PL.run(s, 0, 3)
    assert len(r["verify"]["edges"]) == 20 and all(k.all() for k in r["verify"]["keep"])      # both bridges pass verification
    assert np.diff(r["rounds"][0]["tracks"]["trk_off"]).tolist() == [12] and SR.track_conflicts(r["rounds"][0]["tracks"]).tolist() == [4]
    assert [x["tracks"] is not None for x in r["rounds"]] == [True, True, False] and r["rounds"][2]["n_live"] == 0
    assert np.diff(r["rounds"][1]["tracks"]["trk_off"]).tolist() == [4, 4] and r["rounds"][1]["n_live"] == 12
    xyz, rnd = PL.points(r)
    assert rnd.tolist() == [0, 1, 1] and len(PL.points(PL.run(s, 0, 0))[0]) == 1
    eps = np.sqrt(2.0) * (s["noise"] + 2.0 ** -14)
    owner = np.linalg.norm(xyz[:, None] - s["xyz"][None], axis=2).argmin(1)
    assert sorted(owner.tolist()) == [0, 1, 2] and owner[0] == 1
    for k, p in enumerate(owner.tolist()):
        bound, _ = _bound(s, p, s["point_rows"][p], eps, True)
        d = float(np.linalg.norm(xyz[k] - s["xyz"][p]))
        print(f"chain: point {p} in round {rnd[k]}, |X - X*| = {d:.4f}, bound {bound:.4f}")
        assert d <= bound
    assert (r["rounds"][2]["state"] == PL.TAKEN).all()


def test_rows_of_a_track_that_is_not_accepted_are_dead_for_good():
    s = PL.dead_scene()
    r = PL.run(s, 0, 2)
    far = s["point_rows"][PL.FAR]
    t0 = r["rounds"][0]
    assert t0["tri"]["accept"].tolist() == [True, False] and sorted(t0["tracks"]["trk_row"][8:].tolist()) == sorted(far)
    assert t0["tri"]["traces"][1]["low_angle"] == 1 and t0["tri"]["best"][1] == -1
    for x in r["rounds"][1:]:
        assert (x["state"][far] == PL.DEAD).all() and not np.isin(x["edges"], far).any()
        assert x["tracks"] is None or not np.isin(x["tracks"]["trk_row"], far).any()
    assert len(PL.points(r)[0]) == 2 and r["rounds"][1]["n_live"] == 6 and r["rounds"][2]["n_live"] == 0 and r["rounds"][2]["tracks"] is None


def test_leftovers_of_one_row_and_of_one_frame_end_the_rounds():
    for n_lone in (1, 2):
        s = PL.lone_scene(n_lone)
        r = PL.run(s, 0, 3)
        lone = [s["point_rows"][1 + k][0] for k in range(n_lone)]
        assert all(k.all() for k in r["verify"]["keep"]) and np.diff(r["rounds"][0]["tracks"]["trk_off"]).tolist() == [4 + n_lone]
        assert len(r["rounds"]) == 2 and r["rounds"][1]["n_live"] == 0 and r["rounds"][1]["tracks"] is None
        assert np.nonzero(r["rounds"][1]["state"] == PL.FREE)[0].tolist() == sorted(lone) and len(PL.points(r)[0]) == 1
    # an edge between the two leftover rows of one frame: a track that stage 4 cannot accept, DEAD in the round after
    edges = np.concatenate([r["edges"], [lone]])
    x = PL.rounds(s, edges, 3)
    assert [y["n_live"] for y in x[1:]] == [1, 0] and x[1]["tracks"]["trk_row"].tolist() == sorted(lone)
    assert x[1]["tri"]["accept"].tolist() == [False] and x[1]["tri"]["traces"][0]["same_frame"] == 1
    assert (x[2]["state"][lone] == PL.DEAD).all() and x[2]["tracks"] is None


# ---------------------------------------------------------------- the simulation
def _distinct_per_round(s, r) -> list:
    out, found = [], set()
    for x in PL.complete(r):
        found |= PL.distinct_found(s, x["tri"]["xyz"][x["tri"]["accept"]])
        out.append(len(found))
    return out


def test_clean_matches_give_no_further_track():
    s = SR.sweep_scene(0.0, PL.SWEEP_SEED)
    for ms in (0, 1):
        r = PL.run(s, ms, 2)
        assert len(PL.complete(r)) == 1 and r["rounds"][1]["tracks"] is None and len(r["rounds"]) == 2
        assert len(PL.points(r)[0]) == int(r["tri"]["accept"].sum()) == 200
        print(f"p = 0, min_support = {ms}: {_distinct_per_round(s, r)[0]} of 200 found, {r['rounds'][1]['n_live']} live edges in round 1")


@pytest.mark.parametrize("name,more", [("sweep05", 15), ("sweep10", 35)])
def test_sweep_recovers_planted_points_round_by_round(name, more):
    """Measured, 200 points, 20 frames, seed 1, min_support = 1, distinct planted points found after each round:
    p = 5 %: 165, 182, 186; p = 10 %: 130, 158, 167, 173, 176."""
    s, ms, R, r = PL.gpu_run(name)
    d = _distinct_per_round(s, r)
    print(f"{name}: min_support = {ms}, distinct planted points found after each round {d}; live edges {[x['n_live'] for x in r['rounds'][1:]]}")
    assert len(d) == R + 1 and d[-1] >= d[0] + more and all(b >= a for a, b in zip(d[:-1], d[1:]))
    # a row has one point at most: no round's table holds a row an earlier round kept
    taken = set()
    for x in PL.complete(r):
        rows = x["tracks"]["trk_row"]
        assert not taken & set(rows.tolist())
        keep = x["tri"]["entry_keep"] & np.repeat(x["tri"]["accept"], np.diff(x["tracks"]["trk_off"]))
        taken |= set(rows[keep].tolist())


def test_one_giant_component_gives_about_a_point_per_round():
    s = SR.sweep_scene(0.10, PL.SWEEP_SEED)
    r = PL.run(s, 0, 2)
    d = _distinct_per_round(s, r)
    print(f"p = 10 %, min_support = 0: largest component {int(np.diff(r['tracks']['trk_off']).max())} rows, found after each round {d}")
    assert np.diff(r["tracks"]["trk_off"]).max() >= 800 and d[-1] - d[0] <= 4


# ---------------------------------------------------------------- the margins of every round the GPU test runs
@pytest.mark.parametrize("name", sorted(PL.GPU_RUNS))
def test_margins_the_gpu_test_relies_on(name):
    s, ms, R, r = PL.gpu_run(name)
    v = r["verify"]
    for e, th, ok in zip(v["errors"], v["thresholds"], v["in_range"]):
        for c in range(2):
            assert np.all(np.abs(e[ok, c] - th[c]) > 1e-9 * th[c])
    if ms:
        tr = r["support"]["trace"]
        assert not (np.abs(tr["err"][tr["reached"]] - MAX_REPROJ) <= 1e-6).any() and not (np.abs(tr["angles"].max(1) - MIN_ANGLE) <= 1e-9).any()
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert not (np.abs(tr["angles"][:, a] - tr["angles"][:, b]) <= 1e-12).any()
    tracks = 0
    for k, x in enumerate(PL.complete(r)):
        for tr in x["tri"]["traces"]:
            tracks += 1
            assert all(abs(y - MAX_REPROJ) > 1e-6 for y in tr["reproj"]), (name, k)
            assert all(abs(y - MIN_ANGLE) > 1e-9 for y in tr["angles"]), (name, k)
            hyps = [h for h in tr["hyps"] if h[3] >= 2]
            for n, (_, i, j, cnt, sse) in enumerate(hyps):
                for _, i2, j2, cnt2, sse2 in hyps[n + 1:]:
                    if cnt == cnt2 and (i, j) != (i2, j2):      # the same pair drawn twice ties exactly, by construction
                        assert abs(sse - sse2) > 1e-9 * max(sse, sse2), (name, k, tr["L"], i, j, i2, j2)
                    if (i, j) == (i2, j2):
                        assert cnt == cnt2 and sse == sse2
    print(f"{name}: {tracks} tracks over {len(PL.complete(r))} rounds")


# ---------------------------------------------------------------- the host side, ops replaced by the restatement
class SplitStub(StubOps):
    TRI_ROW_FREE, TRI_ROW_TAKEN, TRI_ROW_DEAD = PL.FREE, PL.TAKEN, PL.DEAD
    extra_live = 0

    def tri_split(self, trk_off, trk_row, T, E, accept, entry_keep, edges, n_edges, n_rows, state=None):
        self.calls.append("tri_split")
        trk = {"trk_off": trk_off.numpy()[:T + 1], "trk_row": trk_row.numpy()[:E]}
        tri = {"accept": accept.numpy()[:T].astype(bool), "entry_keep": entry_keep.numpy()[:E].astype(bool)}
        r = PL.split(n_rows, trk, tri, edges.numpy()[:n_edges], None if state is None else state.numpy()[:n_rows])
        return {"state": self._t(r["state"]), "edges": self._t(r["edges"]), "n_live": torch.tensor([r["n_live"] + self.extra_live], dtype=torch.int32)}


@pytest.fixture()
def stubbed(monkeypatch):
    from pram_amd.localization import triangulation as TG
    stub = SplitStub()
    monkeypatch.setattr(TG, "ops", stub)
    monkeypatch.setattr(TG, "_device", lambda device: torch.device("cpu"))
    return TG, stub


TODAY = {"point_ids", "point3D_xyzs", "track_error", "tracks", "point3D_frame_ids", "frames", "pair_index", "inlier_ratio"}
ROUND = ["tri_split", "tri_components", "tri_tracks", "tri_triangulate"]


def _after_round_0(calls: list) -> list:
    return calls[calls.index("tri_triangulate") + 1:]


def test_host_logic_with_ops_stubbed(stubbed):
    TG, stub = stubbed
    assert TG.SPLIT_DEFAULTS == {"split_rounds": 0} and TG.SUPPORT_DEFAULTS == {"min_support": 0} and set(TG.DEFAULTS) == set(TR.DEFAULTS)
    s = SR.glued_scene()
    # ---- the default never reaches the new entry
    for params in ({}, {"split_rounds": 0}):
        stub.calls.clear()
        m0 = _map(TG, s, **params)
        assert "tri_split" not in stub.calls and set(m0) == TODAY and len(m0["point_ids"]) == 1
    # ---- one round: the four calls in order, the second point, the new keys
    stub.calls.clear()
    m = _map(TG, s, split_rounds=1)
    assert _after_round_0(stub.calls) == ROUND and set(m) == TODAY | {"point_round", "split"}
    want = PL.run(s, 0, 1)
    assert np.array_equal(m["point3D_xyzs"], PL.points(want)[0]) and m["point_round"].tolist() == [0, 1] and m["point_round"].dtype == np.int32
    assert m["point_ids"].tolist() == [1, 2] and np.array_equal(m["point3D_xyzs"][:1], m0["point3D_xyzs"]) and np.array_equal(m["track_error"][:1], m0["track_error"])
    assert all(np.array_equal(a, b) for a, b in zip(m["tracks"][1], m0["tracks"][1])) and [len(t[0]) for t in m["tracks"].values()] == [4, 4]
    assert {k: v.tolist() for k, v in m["split"].items()} == {"live_edges": [6], "tracks": [1], "points": [1]}
    assert sorted(np.concatenate([f["point3D_ids"] for f in m["frames"]]).tolist()) == [1] * 4 + [2] * 4
    for f, fr in enumerate(m["frames"]):
        assert np.array_equal(fr["xyzs"], m["point3D_xyzs"][fr["point3D_ids"] - 1])
    # ---- a cap beyond what is left: the round that finds no edge is the last, and it runs no stage
    stub.calls.clear()
    m3 = _map(TG, s, split_rounds=5)
    assert _after_round_0(stub.calls) == ROUND + ["tri_split"] and m3["split"]["live_edges"].tolist() == [6, 0]
    assert m3["split"]["tracks"].tolist() == [1, 0] and m3["split"]["points"].tolist() == [1, 0] and np.array_equal(m3["point3D_xyzs"], m["point3D_xyzs"])
    # ---- a leftover without an edge: the first further round is the last
    stub.calls.clear()
    m1 = _map(TG, PL.lone_scene(2), split_rounds=4)
    assert _after_round_0(stub.calls) == ["tri_split"] and m1["split"]["live_edges"].tolist() == [0] and len(m1["point_ids"]) == 1
    # ---- an edge but no track (a loop is the only such edge; the stub reports one more than there is): the rounds stop after the tracks
    stub.calls.clear()
    stub.extra_live = 1
    m1 = _map(TG, PL.lone_scene(2), split_rounds=4)
    stub.extra_live = 0
    assert _after_round_0(stub.calls) == ROUND[:3] and len(m1["point_ids"]) == 1
    assert {k: v.tolist() for k, v in m1["split"].items()} == {"live_edges": [1], "tracks": [0], "points": [0]}
    # ---- several rounds with stage 2b, against the restatement
    sw = SR.sweep_scene(0.05, PL.SWEEP_SEED)
    stub.calls.clear()
    m = _map(TG, sw, min_support=1, split_rounds=2)
    want = PL.run(sw, 1, 2)
    xyz, rnd = PL.points(want)
    assert _after_round_0(stub.calls) == ROUND * 2 and stub.calls.count("tri_support") == 1
    assert np.array_equal(m["point3D_xyzs"], xyz) and np.array_equal(m["point_round"], rnd) and m["point_ids"].tolist() == list(range(1, len(xyz) + 1))
    assert m["split"]["live_edges"].tolist() == [x["n_live"] for x in want["rounds"][1:]] and "support" in m
    assert m["split"]["points"].tolist() == [int((rnd == k).sum()) for k in (1, 2)] and m["split"]["tracks"].tolist() == [len(x["tracks"]["trk_label"]) for x in want["rounds"][1:]]
    pid = np.concatenate([f["point3D_ids"] for f in m["frames"]])
    assert (pid >= 1).sum() == sum(len(t[0]) for t in m["tracks"].values())      # no row has two points
    # ---- split_edges on its own, round after round
    table = TG.frame_table(sw["frames"], sw["cameras"], (sw["qvec"], sw["tvec"]), "cpu")
    state = None
    for x, nxt in zip(PL.complete(want), want["rounds"][1:]):
        got = TG.split_edges(table, want["edges"], x["tracks"], x["tri"], state)
        assert got["state"].dtype == np.uint8 and got["edges"].dtype == np.int32 and got["n_live"] == nxt["n_live"]
        assert np.array_equal(got["state"], nxt["state"]) and np.array_equal(got["edges"], nxt["edges"])
        state = got["state"]
    with pytest.raises(ValueError):
        TG.split_edges(table, want["edges"], want["tracks"], want["tri"], state[:-1])
    # ---- refusals
    for value in (-1, 1.5):
        with pytest.raises(ValueError):
            _map(TG, s, split_rounds=value)
    with pytest.raises(TypeError):
        _map(TG, s, split_round=1)
    for word in ("split_rounds", "FREE", "TAKEN", "DEAD", "per round", "glued"):
        assert word in TG.__doc__, word


def test_map_tables_numbers_from_an_offset_and_split_tables_joins_the_rounds():
    from pram_amd.localization import triangulation as TG
    s, ms, R, r = PL.gpu_run("sweep05")
    done = PL.complete(r)
    ids = np.arange(s["n_frames"])
    a = TG.map_tables(ids, s["frame_off"], done[0]["tracks"], done[0]["tri"])
    b = TG.map_tables(ids, s["frame_off"], done[0]["tracks"], done[0]["tri"], first_id=10)
    assert a["point_ids"][0] == 1 and np.array_equal(b["point_ids"], a["point_ids"] + 9) and list(b["tracks"]) == b["point_ids"].tolist()
    m = TG.split_tables(ids, s["frame_off"], [(x["tracks"], x["tri"]) for x in done])
    P0 = len(a["point_ids"])
    assert np.array_equal(m["point_ids"], np.arange(1, len(m["point_ids"]) + 1)) and np.array_equal(m["point_round"], PL.points(r)[1])
    for k in ("point_ids", "point3D_xyzs", "track_error"):
        assert m[k][:P0].tobytes() == a[k].tobytes() and m[k].dtype == a[k].dtype
    assert all(np.array_equal(m["tracks"][p][0], a["tracks"][p][0]) and np.array_equal(m["tracks"][p][1], a["tracks"][p][1]) for p in a["tracks"])
    for f, (fm, fa) in enumerate(zip(m["frames"], a["frames"])):
        was = fa["point3D_ids"] >= 1
        assert np.array_equal(fm["point3D_ids"][was], fa["point3D_ids"][was]) and (fm["point3D_ids"][~was] > P0).sum() == ((fm["point3D_ids"] > P0).sum())
        has = fm["point3D_ids"] >= 1
        assert np.array_equal(fm["xyzs"][has], m["point3D_xyzs"][fm["point3D_ids"][has] - 1]) and not fm["xyzs"][~has].any()
    one = TG.split_tables(ids, s["frame_off"], [(done[0]["tracks"], done[0]["tri"])])
    assert not one["point_round"].any() and all(one[k].tobytes() == a[k].tobytes() for k in ("point_ids", "point3D_xyzs", "track_error"))
