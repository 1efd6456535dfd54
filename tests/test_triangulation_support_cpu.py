"""CPU: stage 2b of the triangulation, third-view support of every match (tests/triangulation_support_ref.py): the restatement
against a brute-force count written with sets, the margins that make the device's counts exact on the scenes the GPU test uses,
the glued scene that pins the weakness the stage is for, the simulation at a size the CPU runs in seconds, and the host side of
pram_amd.localization.triangulation with ops replaced by the restatement."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import triangulation_ref as TR
from tests import triangulation_support_ref as SR
from tests.test_triangulation_cpu import _bound

MIN_ANGLE = float(np.deg2rad(SR.DEFAULTS["min_tri_angle"]))
MAX_REPROJ = SR.DEFAULTS["max_reproj_error"]
SWEEP_SEEDS = (1, 2, 3)


def verified_edges(s: dict) -> np.ndarray:
    use = TR.unique_pairs(s["pairs"])
    return TR.verify(s["norm0"], s["frame_off"], s["table"], s["pairs"][use], [s["matches"][i] for i in use])["edges"]


def gpu_cases() -> dict:
    """name -> (scene, edges): what tests/test_gpu_triangulation_support.py runs the support kernel on."""
    star, glued, tri, sweep = SR.star_scene(), SR.glued_scene(), TR.tri_scene(), SR.sweep_scene(0.05, SWEEP_SEEDS[0])
    return {"star": (star, star["edges"]), "glued": (glued, verified_edges(glued)), "tri": (tri, verified_edges(tri)),
            "sweep": (sweep, verified_edges(sweep))}


def test_symbols_declared_and_exported(hip_lib):
    # the entries' declarations, types and exports: tests/test_abi_contract_cpu.py
    from pram_amd import _lib, ops
    assert {"pram_tri_adjacency_workspace_bytes", "pram_tri_adjacency", "pram_tri_support"} <= set(_lib.exported_symbols())
    assert callable(ops.tri_adjacency) and callable(ops.tri_support)


# ---------------------------------------------------------------- the independent count
def brute_support(s: dict, edges) -> np.ndarray:
    """Neighbour sets instead of a CSR, plain floats instead of arrays for the angles, the choice of the pair and the midpoint;
    the inlier test is TR.Track's."""
    n = int(s["frame_off"][-1])
    frame = (np.searchsorted(np.asarray(s["frame_off"]), np.arange(n), side="right") - 1).tolist()
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist()
    counts = lambda u, v: 0 <= u < n and 0 <= v < n and u != v
    nb: dict = {}
    for u, v in edges:
        if counts(u, v):
            nb.setdefault(u, set()).add(v)
            nb.setdefault(v, set()).add(u)
    tk = SR.all_rows(s)
    ray, C = tk.ray.tolist(), tk.C.tolist()
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def angle(a, b):
        c = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        return math.atan2(math.sqrt(dot(c, c)), dot(a, b))

    triples, Xs = [], []
    for i, (u, v) in enumerate(edges):
        if not counts(u, v) or frame[u] == frame[v]:
            continue
        for w in sorted((nb[u] | nb[v]) - {u, v}):
            if frame[w] in (frame[u], frame[v]):
                continue
            prs = ((u, v), (u, w), (v, w))
            ang = [angle(ray[a], ray[b]) for a, b in prs]
            a, b = prs[ang.index(max(ang))]
            if not max(ang) >= MIN_ANGLE:
                continue
            C1, d1, C2, d2 = C[a], ray[a], C[b], ray[b]
            wv = [C1[k] - C2[k] for k in range(3)]
            aa, bb, cc, dd, ee = dot(d1, d1), dot(d1, d2), dot(d2, d2), dot(d1, wv), dot(d2, wv)
            den = aa * cc - bb * bb
            if den == 0.0:
                continue      # no scene here has parallel rays above the angle bar; the arrays would give NaN, no inlier
            sp, up = (bb * ee - cc * dd) / den, (aa * ee - bb * dd) / den
            Xs.append([0.5 * ((C1[k] + sp * d1[k]) + (C2[k] + up * d2[k])) for k in range(3)])
            triples.append((i, u, v, w))
    sup = np.zeros(len(edges), dtype=np.int32)
    if triples:
        tr, X = np.array(triples), np.array(Xs).T
        inl = [SR._sub(tk, tr[:, k]).inliers(X, MAX_REPROJ * MAX_REPROJ)[0] for k in (1, 2, 3)]
        sup = np.bincount(tr[inl[0] & inl[1] & inl[2], 0], minlength=len(edges)).astype(np.int32)
    return sup


def test_restatement_equals_the_brute_force_count():
    cases = [("star", SR.star_scene(), SR.star_scene()["edges"])]
    cases += [(f"sweep {seed}", s, verified_edges(s)) for seed in SWEEP_SEEDS for s in (SR.sweep_scene(0.05, seed),)]
    for name, s, e in cases:
        got = SR.support(s, e)
        want = brute_support(s, e)
        print(f"{name}: {len(e)} edges, {len(got['trace']['edge'])} triples, support up to {want.max()}, {int((want == 0).sum())} edges without")
        assert np.array_equal(got["support"], want), name
        assert np.array_equal(got["keep"], want >= 1) and np.array_equal(got["edges"], np.where((want >= 1)[:, None], e, -1))


def test_adjacency_is_sorted_and_depends_on_the_edge_set_alone():
    s = SR.star_scene()
    n = int(s["frame_off"][-1])
    a = SR.adjacency(n, s["edges"], s["frame_off"])
    e = s["edges"][SR.valid_edges(n, s["edges"])]
    assert a["adj_off"][-1] == 2 * len(e) == len(a["adj"]) and len(e) == len(s["edges"]) - 5
    for r in range(n):
        lst = a["adj"][a["adj_off"][r]:a["adj_off"][r + 1]].tolist()
        assert lst == sorted([int(v) for u, v in e.tolist() if u == r] + [int(u) for u, v in e.tolist() if v == r])
    assert np.array_equal(s["frame_off"][a["row_frame"]] <= np.arange(n), np.ones(n, dtype=bool)) and a["row_frame"][-1] == SR.STAR_FRAMES - 1
    again = SR.adjacency(n, s["edges"][np.random.RandomState(0).permutation(len(s["edges"]))][:, ::-1], s["frame_off"])
    assert all(np.array_equal(a[k], again[k]) for k in a)


def test_star_scene_holds_every_case():
    s = SR.star_scene()
    n = int(s["frame_off"][-1])
    r = SR.support(s, s["edges"])
    deg = np.diff(r["adj"]["adj_off"])
    rf, tr, T = r["adj"]["row_frame"], r["trace"], s["tested"]
    idx = {k: SR.edge_index(s, uv) for k, uv in T.items()}
    sup = {k: int(r["support"][i]) for k, i in idx.items()}
    length = {k: int(deg[u] + deg[v]) for k, (u, v) in T.items() if SR.valid_edges(n, [(u, v)])[0]}
    assert deg[s["hub"]] == 200 and deg[s["lonely"]] == 0 and length["hub"] >= 200
    assert SR.STAR_LENGTHS <= set(length.values()) and all(length[f"len{x}"] == x for x in SR.STAR_LENGTHS)
    assert sup["none"] == sup["past_the_end"] == sup["loop"] == 0 and not r["keep"][[idx["none"], idx["past_the_end"], idx["loop"]]].any()
    assert sup["len2"] == 0 and sup["len3"] == 1 and sup["len130"] == 0 and sup["hub"] >= 60
    assert all(sup[f"len{x}"] >= 50 for x in (63, 64, 65, 66, 67))
    # a match given twice: both copies get the same count and the witness lists hold no row twice
    assert (s["edges"] == np.asarray(T["duplicate"])).all(1).sum() == 1 and sup["duplicate"] == sup["duplicate_reversed"] >= 50
    u, v = T["len64"]
    lu = r["adj"]["adj"][r["adj"]["adj_off"][u]:r["adj"]["adj_off"][u + 1]]
    assert len(lu) == len(set(lu.tolist())) + 1      # the duplicate stands twice in the hub of the star
    for k in idx.values():
        w = tr["rows"][tr["edge"] == k][:, 2].tolist()
        assert len(w) == len(set(w))
    # the triangle's third row is in both lists and is one witness
    u, v = T["triangle"]
    both = set(r["adj"]["adj"][r["adj"]["adj_off"][u]:r["adj"]["adj_off"][u + 1]].tolist()) & set(r["adj"]["adj"][r["adj"]["adj_off"][v]:r["adj"]["adj_off"][v + 1]].tolist())
    assert len(both) == 1 and (tr["rows"][tr["edge"] == idx["triangle"]][:, 2] == both.pop()).sum() == 1
    # a neighbour in the frame of one end is no witness; two rows of one frame are no edge to support
    u, v = T["same_frame_neighbour"]
    nv = r["adj"]["adj"][r["adj"]["adj_off"][v]:r["adj"]["adj_off"][v + 1]]
    assert (rf[nv[nv != u]] == rf[u]).sum() == 1 and not (rf[tr["rows"][tr["edge"] == idx["same_frame_neighbour"]][:, 2]] == rf[u]).any()
    u, v = T["same_frame_edge"]
    assert rf[u] == rf[v] and deg[u] + deg[v] >= 3 and sup["same_frame_edge"] == 0 and not (tr["edge"] == idx["same_frame_edge"]).any()
    # low parallax: the edge's own rays meet under less than min_tri_angle, a third view with baseline confirms it through another pair
    m = tr["edge"] == idx["low_parallax"]
    assert m.sum() == 1 and tr["angles"][m][0, 0] < MIN_ANGLE < tr["angles"][m][0].max() and tr["pick"][m][0] != 0 and sup["low_parallax"] == 1
    m = tr["edge"] == idx["low_parallax_triple"]
    assert m.sum() == 1 and tr["angles"][m].max() < MIN_ANGLE and not tr["reached"][m].any() and sup["low_parallax_triple"] == 0
    assert set(tr["pick"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("name", ["star", "glued", "tri", "sweep"])
def test_margins_the_gpu_test_relies_on(name):
    s, e = gpu_cases()[name]
    tr = SR.support(s, e)["trace"]
    err = tr["err"][tr["reached"]]
    assert len(tr["edge"]) > 0 and not (np.abs(err - MAX_REPROJ) <= 1e-6).any()
    best = tr["angles"].max(1)
    assert not (np.abs(best - MIN_ANGLE) <= 1e-9).any()
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not (np.abs(tr["angles"][:, a] - tr["angles"][:, b]) <= 1e-12).any()


# ---------------------------------------------------------------- the glued scene
def _point_of(s, r, p):
    """The accepted track that holds planted point p's rows, and those rows."""
    rows = [int(s["frame_off"][f]) + s["where"][(f, p)] for f in s["seen"][p]]
    lab = r["tracks"]["trk_label"]
    t = int(np.searchsorted(lab, r["label"][rows[0]]))
    assert t < len(lab) and lab[t] == r["label"][rows[0]] and all(r["label"][x] == lab[t] for x in rows)
    return t, rows


def test_glued_scene_one_point_without_the_filter_two_with():
    s = SR.glued_scene()
    before, after = SR.run(s, 0), SR.run(s, 1)
    e = before["verify"]["edges"]
    assert len(e) == 13 and all(k.all() for k in before["verify"]["keep"])      # the bridge passes verification
    bridge = e.tolist().index(list(s["bridge"]))
    sup = after["support"]["support"]
    assert sup[bridge] == 0 and (np.delete(sup, bridge) >= 1).all() and after["support"]["keep"].sum() == 12
    # the weakness: one component of eight rows, two entries in each of two frames, one point
    assert np.diff(before["tracks"]["trk_off"]).tolist() == [8] and before["tri"]["accept"].tolist() == [True] and before["tri"]["kept"][0] == 4
    assert SR.track_conflicts(before["tracks"]).tolist() == [2]
    assert np.diff(after["tracks"]["trk_off"]).tolist() == [4, 4] and after["tri"]["accept"].tolist() == [True, True]
    assert SR.track_conflicts(after["tracks"]).tolist() == [0, 0]
    eps = np.sqrt(2.0) * (s["noise"] + 2.0 ** -14)
    for p in (0, 1):
        t, rows = _point_of(s, after, p)
        bound, _ = _bound(s, p, rows, eps, True)
        d = float(np.linalg.norm(after["tri"]["xyz"][t] - s["xyz"][p]))
        print(f"point {p}: |X - X*| = {d:.4f}, bound {bound:.4f}")
        assert after["tri"]["kept"][t] == 4 and d <= bound


# ---------------------------------------------------------------- the simulation
def _stats(s, r) -> dict:
    e = r["verify"]["edges"]
    true = s["owner"][e[:, 0]] == s["owner"][e[:, 1]]
    keep = r["support"]["keep"] if r["support"] is not None else np.ones(len(e), dtype=bool)
    sizes = np.diff(r["tracks"]["trk_off"])
    return {"edges": len(e), "wrong": int((~true).sum()), "true_dropped": int((true & ~keep).sum()), "wrong_kept": int((~true & keep).sum()),
            "tracks": len(sizes), "largest": int(sizes.max()), "accepted": int(r["tri"]["accept"].sum()),
            "conflicting": int((SR.track_conflicts(r["tracks"]) > 0).sum())}


def test_sweep_drops_no_true_match_that_has_a_third_view():
    """Without wrong matches every edge with a neighbour in a third frame keeps its place (measured: 2631 edges, all kept)."""
    s = SR.sweep_scene(0.0, SWEEP_SEEDS[0])
    r = SR.run(s, 1)
    e, sup = r["verify"]["edges"], r["support"]
    assert len(e) == s["n_true"] and s["n_wrong"] == 0
    has_witness = np.isin(np.arange(len(e)), sup["trace"]["edge"])
    print(f"p = 0: {len(e)} edges, {int(has_witness.sum())} with a third-view neighbour, {int((has_witness & ~sup['keep']).sum())} of them dropped")
    assert has_witness.sum() >= 0.9 * len(e) and not (has_witness & ~sup["keep"]).any()


@pytest.mark.parametrize("p", [0.02, 0.05])
def test_sweep_more_points_and_no_more_conflicts_with_the_filter(p):
    """Measured, 200 points, 20 frames, seed 1 (tracks / largest / accepted / conflicting tracks, without -> with min_support = 1):
    p = 2 %: 148 / 72 / 148 / 23 -> 187 / 23 / 187 / 9, 0 true matches dropped, 13 of 53 wrong ones kept;
    p = 5 %:  80 / 277 / 80 / 18 -> 176 / 29 / 176 / 16, 0 true matches dropped, 24 of 132 wrong ones kept."""
    s = SR.sweep_scene(p, SWEEP_SEEDS[0])
    a, b = _stats(s, SR.run(s, 0)), _stats(s, SR.run(s, 1))
    print(f"p = {p}: without {a}\n          with    {b}")
    assert a["wrong"] == s["n_wrong"] > 0 and b["accepted"] > a["accepted"] and b["conflicting"] <= a["conflicting"]


# ---------------------------------------------------------------- the host side, ops replaced by the restatement
class StubOps:
    """pram_amd.ops' triangulation wrappers on CPU tensors, computed by the restatement; ``calls`` records the names."""
    TRI_CC_STATE_WORDS, TRI_CC_DONE = 4, 1

    def __init__(self):
        self.calls = []

    @staticmethod
    def _t(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a if a.shape[0] else np.zeros((1,) + a.shape[1:], dtype=a.dtype))

    def tri_frames(self, qvec, tvec, cam_model, cam_params, host):
        F = len(host)
        self.calls.append("tri_frames")
        return self._t(TR.frame_table(qvec.numpy()[:F], tvec.numpy()[:F], cam_model.numpy()[:F], cam_params.numpy()[:F]))

    def tri_normalize(self, keypoints, frame_off, cam_model, cam_params, host, n_rows, off):
        F = len(host)
        self.calls.append("tri_normalize")
        return self._t(TR.normalize(keypoints.numpy()[:n_rows], frame_off.numpy()[:F + 1], cam_model.numpy()[:F], cam_params.numpy()[:F], off))

    def tri_verify(self, norm, frame_off, pairs, match_off, matches, table, F, Pn, M, max_error):
        self.calls.append("tri_verify")
        off, m = match_off.numpy()[:Pn + 1], matches.numpy()[:M]
        v = TR.verify(norm.numpy(), frame_off.numpy()[:F + 1], table.numpy(), pairs.numpy()[:Pn], [m[a:b] for a, b in zip(off[:-1], off[1:])], max_error)
        keep = np.concatenate(v["keep"] + [np.zeros(0, dtype=bool)])
        edges, kept = np.full((M, 2), -1, dtype=np.int32), np.zeros((M, 2), dtype=np.int32)
        edges[keep] = v["edges"]
        for a, k in zip(off[:-1], v["kept"]):
            kept[a:a + len(k)] = k
        return {"keep": self._t(keep.astype(np.uint8)), "kept": self._t(kept), "edges": self._t(edges), "count": self._t(np.array(v["count"], dtype=np.int32))}

    def tri_components(self, edges, n_edges, n_rows, first, n_rounds, label, state):
        self.calls.append("tri_components")
        label[:n_rows] = torch.from_numpy(TR.components(n_rows, edges.numpy()[:n_edges]))[:n_rows]
        state[self.TRI_CC_DONE] = 1

    def tri_tracks(self, label, frame_off, F, n):
        self.calls.append("tri_tracks")
        t = TR.tracks(label.numpy()[:n], frame_off.numpy()[:F + 1])
        return {**{k: self._t(v) for k, v in t.items()}, "sizes": torch.tensor([len(t["trk_label"]), len(t["trk_row"])], dtype=torch.int32)}

    def tri_triangulate(self, norm, keypoints, table, cam_model, cam_params, trk_off, trk_label, trk_row, trk_frame, T, E, F, n, **p):
        self.calls.append("tri_triangulate")
        s = {"table": table.numpy(), "cam_model": cam_model.numpy(), "cam_params": cam_params.numpy(), "keypoints": keypoints.numpy(), "norm05": norm.numpy()}
        trk = {"trk_off": trk_off.numpy()[:T + 1], "trk_label": trk_label.numpy()[:T], "trk_row": trk_row.numpy()[:E], "trk_frame": trk_frame.numpy()[:E]}
        r = TR.triangulate(s, trk, trials=p["trials"], seed=p["seed"], min_tri_angle=float(np.rad2deg(p["min_tri_angle"])), max_reproj_error=p["max_reproj_error"])
        return {"accept": self._t(r["accept"].astype(np.int32)), "xyz": self._t(r["xyz"]), "error": self._t(r["error"]), "kept": self._t(r["kept"]),
                "best": self._t(r["best"]), "entry_keep": self._t(r["entry_keep"].astype(np.uint8)), "entry_error": self._t(r["entry_error"])}

    def tri_adjacency(self, edges, n_edges, frame_off, F, n):
        self.calls.append("tri_adjacency")
        self.frame_off = frame_off.numpy()[:F + 1]
        return {k: self._t(v) for k, v in SR.adjacency(n, edges.numpy()[:n_edges], self.frame_off).items()}

    def tri_support(self, norm, keypoints, table, cam_model, cam_params, edges, n_edges, adj_off, adj, row_frame, F, n, min_tri_angle, max_reproj_error,
                    min_support):
        self.calls.append("tri_support")
        s = {"table": table.numpy(), "cam_model": cam_model.numpy(), "cam_params": cam_params.numpy(), "keypoints": keypoints.numpy()[:n],
             "norm05": norm.numpy()[:n], "frame_off": self.frame_off}
        r = SR.support(s, edges.numpy()[:n_edges], min_support, float(np.rad2deg(min_tri_angle)), max_reproj_error)
        return {"support": self._t(r["support"]), "edges": self._t(r["edges"])}


@pytest.fixture()
def stubbed(monkeypatch):
    from pram_amd.localization import triangulation as TG
    stub = StubOps()
    monkeypatch.setattr(TG, "ops", stub)
    monkeypatch.setattr(TG, "_device", lambda device: torch.device("cpu"))
    return TG, stub


def _map(TG, s, **params):
    return TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], s["matches"], "cpu", **params)


TODAY = {"point_ids", "point3D_xyzs", "track_error", "tracks", "point3D_frame_ids", "frames", "pair_index", "inlier_ratio"}


def test_host_logic_with_ops_stubbed(stubbed):
    TG, stub = stubbed
    s = SR.glued_scene()
    assert TG.SUPPORT_DEFAULTS == {"min_support": 0} and set(TG.DEFAULTS) == set(TR.DEFAULTS) and all(TG.DEFAULTS[k] == TR.DEFAULTS[k] for k in TR.DEFAULTS)
    assert set(TG.VERIFY_DEFAULTS) == {"max_error"} and set(TG.TRI_DEFAULTS) == {"trials", "seed", "min_tri_angle", "max_reproj_error"}
    # ---- the default: neither new wrapper, today's keys, the glued component's one point
    for params in ({}, {"min_support": 0}):
        stub.calls.clear()
        m = _map(TG, s, **params)
        assert "tri_adjacency" not in stub.calls and "tri_support" not in stub.calls and "tri_triangulate" in stub.calls
        assert set(m) == TODAY and len(m["point_ids"]) == 1
    # ---- min_support = 1: both wrappers once, between verification and the components; two points; the support lists
    stub.calls.clear()
    m = _map(TG, s, min_support=1)
    order = [c for c in stub.calls if c in ("tri_verify", "tri_adjacency", "tri_support", "tri_components")]
    assert order[:4] == ["tri_verify", "tri_adjacency", "tri_support", "tri_components"] and stub.calls.count("tri_support") == 1
    want = SR.run(s, 1)
    assert set(m) == TODAY | {"support"} and len(m["point_ids"]) == 2 and np.array_equal(m["point3D_xyzs"], want["tri"]["xyz"])
    assert [len(x) for x in m["support"]] == [len(s["matches"][i]) for i in m["pair_index"].tolist()] and all(x.dtype == np.int32 for x in m["support"])
    assert np.array_equal(np.concatenate(m["support"]), want["support"]["support"])      # nothing was dropped by verification here
    k04 = m["pair_index"].tolist().index(s["pairs"].tolist().index([0, 4]))
    assert m["support"][k04].tolist() == [0]
    # ---- a match that verification drops reads -1
    bad = [x.copy() for x in s["matches"]]
    bad[0] = np.concatenate([bad[0], [[-1, 0]]])
    m = TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], bad, "cpu", min_support=1)
    assert m["support"][0][-1] == -1 and (m["support"][0][:-1] >= 1).all() and len(m["point_ids"]) == 2
    # ---- refusals
    for params in ({"min_supports": 1}, {"support": 1}):
        with pytest.raises(TypeError):
            _map(TG, s, **params)
    for value in (-1, 1.5):
        with pytest.raises(ValueError):
            _map(TG, s, min_support=value)
    with pytest.raises(TypeError):
        TG.support_matches({}, np.zeros((0, 2)), trials=3)
    # ---- support_matches and adjacency on their own
    table = TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), "cpu")
    e = want["verify"]["edges"]
    got = TG.support_matches(table, e)
    assert got["support"].dtype == np.int32 and np.array_equal(got["support"], want["support"]["support"]) and got["keep"].dtype == bool
    assert np.array_equal(got["edges"], want["support"]["edges"]) and got["edges"].dtype == np.int32
    assert not TG.support_matches(table, e, min_support=4)["keep"].any()
    a = TG.adjacency(table, e)
    assert all(np.array_equal(a[k], want["support"]["adj"][k]) for k in ("adj_off", "adj", "row_frame"))
    for word in ("min_support", "stage 2b", "glued"):
        assert word in TG.__doc__, word


def test_track_conflicts_against_a_loop():
    from pram_amd.localization import triangulation as TG
    rng = np.random.RandomState(4)
    sizes = [2, 3, 9, 40, 2, 17]
    trk = {"trk_off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
           "trk_frame": np.concatenate([np.sort(rng.randint(0, 12, size=n)) for n in sizes]).astype(np.int32)}
    got = TG.track_conflicts(trk)
    assert got.dtype == np.int64 and np.array_equal(got, SR.track_conflicts(trk)) and got.max() >= 5 and (got == 0).any()
    assert TG.track_conflicts({"trk_off": np.zeros(1, dtype=np.int32), "trk_frame": np.zeros(0, dtype=np.int32)}).shape == (0,)
    for p in (0.0, 0.05):
        r = SR.run(SR.sweep_scene(p, SWEEP_SEEDS[0]), 0)
        got = TG.track_conflicts(r["tracks"])
        assert np.array_equal(got, SR.track_conflicts(r["tracks"])) and (got.any() == (p > 0))
