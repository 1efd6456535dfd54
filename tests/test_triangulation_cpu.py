"""CPU: the numpy restatement of the triangulation stages (tests/triangulation_ref.py) against the reference's own epipolar errors
(tests/golden/triangulation_pinned.npz, tests/tools/gen_triangulation_pinned.py), the branches the planted scene takes, what it
recovers, the margins the GPU test relies on, and the host side of pram_amd.localization.triangulation that needs no GPU."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from tests import pose_ref as PR
from tests import triangulation_ref as TR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_tri_frames", "pram_tri_normalize", "pram_tri_verify", "pram_tri_components", "pram_tri_tracks_workspace_bytes",
           "pram_tri_tracks", "pram_tri_triangulate")
MIN_ANGLE = float(np.deg2rad(TR.DEFAULTS["min_tri_angle"]))
MAX_REPROJ = TR.DEFAULTS["max_reproj_error"]


@pytest.fixture(scope="module")
def noisy():
    s = TR.tri_scene()
    return s, TR.run(s)


@pytest.fixture(scope="module")
def clean():
    s = TR.tri_scene(noise=0.0)
    return s, TR.run(s)


def test_symbols_declared_and_exported(hip_lib):
    from pram_amd import _lib, ops
    header = (ROOT / "include" / "pram_hip.h").read_text()
    # the entries' declarations, types and exports and header == ops for the constants: tests/test_abi_contract_cpu.py
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    assert TR.GN_STEPS == ops.TRI_GN_STEPS and TR.FRAME_COLS == ops.TRI_FRAME_COLS and ops.TRI_CC_STATE_WORDS == 4
    assert int(re.search(r"#define PRAM_POSE_UNDISTORT_STEPS (\d+)", header).group(1)) == PR.UNDISTORT_STEPS
    assert (ROOT / "pram_amd" / "csrc" / "triangulate.hip").exists()
    cam_h, pose = (ROOT / "pram_amd" / "csrc" / "camera.h").read_text(), (ROOT / "pram_amd" / "csrc" / "pose.hip").read_text()
    for helper in ("struct Cam", "cam_unify(int model", "void distort(", "void distort_jac(", "struct V3"):      # moved, not copied
        assert helper in cam_h and helper not in pose, helper


def test_restatement_reproduces_the_reference_errors(golden, noisy):
    """The pinned errors to 1e-12 relative, and the pinned mask exactly.  An error is |x0^T E^T x1| over the norm of a line: nine
    products of order one that cancel to 1e-7 .. 1e-2 on inlier matches.  Two float64 evaluations of it (numpy's matrix products
    in the reference, the kernel's written-out sums here) differ by a few 2^-53 of the sum of the products' magnitudes, whatever
    the sum itself is, so `relative` is taken against that sum: |mine - pinned| <= 1e-12 * pinned * sum|products| / |sum products|.
    Against the pinned value alone the largest deviation is printed: 1.2e-9, at the scene's smallest error, 7.3e-10 (the planted
    match on the epipolar line); at errors of 1e-5, a two-hundredth of a pixel, it is about 1e-11."""
    s, r = noisy
    g = golden("triangulation_pinned")
    rel_literal = (0.0, 0.0)
    assert g["pair_index"].tolist() == r["pair_index"] and np.array_equal(g["pairs"], s["pairs"][r["pair_index"]])
    v = r["verify"]
    for k, (f0, f1) in enumerate(g["pairs"].tolist()):
        a, b = g["match_off"][k], g["match_off"][k + 1]
        ok = v["in_range"][k]
        m = s["matches"][r["pair_index"][k]][ok]
        assert b - a == int(ok.sum())
        # the fixture's inputs are this scene's normalised keypoints
        assert np.array_equal(g["x0"][a:b], s["norm0"][s["frame_off"][f0] + m[:, 0]]) and np.array_equal(g["x1"][a:b], s["norm0"][s["frame_off"][f1] + m[:, 1]])
        E = TR.essential(s["table"][f0], s["table"][f1])
        e0, e1 = TR.epipolar_errors(E, g["x0"][a:b], g["x1"][a:b])
        x0h, x1h = (np.concatenate([g[n][a:b], np.ones((b - a, 1))], 1) for n in ("x0", "x1"))
        dist, terms = np.abs((x0h * (x1h @ E)).sum(1)), (np.abs(x0h) * (np.abs(x1h) @ np.abs(E))).sum(1)
        for mine, ref in ((e0, g["errors"][a:b, 0]), (e1, g["errors"][a:b, 1])):
            assert np.all(np.abs(mine - ref) <= 1e-12 * ref * terms / dist), (k, np.abs(mine - ref).max())
            if b > a:
                rel = np.abs(mine - ref) / np.abs(ref)
                rel_literal = max(rel_literal, (float(rel.max()), float(ref[rel.argmax()])))
        assert np.array_equal(v["keep"][k][ok], g["keep"][a:b]) and not v["keep"][k][~ok].any()
    assert 0 < int(g["keep"].sum()) < len(g["keep"])
    print(f"largest |mine - pinned| / pinned: {rel_literal[0]:.2e}, at an error of {rel_literal[1]:.2e}")


def test_normalisation_inverts_the_camera_model():
    """Every model: the normalised keypoint, distorted and scaled again, is the stored pixel plus the offset."""
    s = TR.tri_scene()
    assert set(s["cam_model"].tolist()) == set(PR.MODELS.values())
    for off, norm in ((0.0, s["norm0"]), (0.5, s["norm05"])):
        for f in range(s["n_frames"]):
            a, b = s["frame_off"][f], s["frame_off"][f + 1]
            fx, fy, cx, cy, k1, k2, p1, p2 = PR.unify(int(s["cam_model"][f]), s["cam_params"][f])
            ud, vd = PR.distort(norm[a:b, 0], norm[a:b, 1], k1, k2, p1, p2)
            px = np.stack([fx * ud + cx, fy * vd + cy], 1)
            assert np.abs(px - (s["keypoints"][a:b].astype(np.float64) + off)).max(initial=0.0) < 1e-9, (off, f)


def _track_of(r, row):
    lab = r["tracks"]["trk_label"]
    t = int(np.searchsorted(lab, r["label"][row]))
    return t if t < len(lab) and lab[t] == r["label"][row] else -1


def test_scene_takes_every_branch(noisy):
    s, r = noisy
    v, trk, tri = r["verify"], r["tracks"], r["tri"]
    row = lambda f, k: int(s["frame_off"][f]) + k
    special, where = s["special"], s["where"]
    pairs = s["pairs"].tolist()
    # ---- the pair list: twice in both orders, an empty pair, a frame without keypoints
    assert [1, 3] in pairs and [3, 1] in pairs and pairs.index([3, 1]) not in r["pair_index"] and pairs.index([1, 3]) in r["pair_index"]
    k_empty = r["pair_index"].index(pairs.index([0, TR.F_EMPTY]))
    assert len(v["keep"][k_empty]) == 0 and v["count"][k_empty] == 0 and s["frame_off"][TR.F_EMPTY] == s["frame_off"][TR.F_EMPTY + 1]
    # ---- wrong matches fail the epipolar test; indices of -1 and of n are dropped
    assert s["n_wrong"] >= 20 and sum(len(k) - int(k.sum()) for k in v["keep"]) >= s["n_wrong"]
    k01 = r["pair_index"].index(pairs.index([0, 1]))
    bad = ~v["in_range"][k01]
    m01 = s["matches"][pairs.index([0, 1])]
    assert bad.sum() == 3 and (m01[bad] == -1).any() and (m01[bad, 1] == s["frame_off"][2] - s["frame_off"][1]).any() and not v["keep"][k01][bad].any()
    # ---- the wrong match on the epipolar line passes verification and falls out at triangulation
    f7, k7 = s["special_rows"]["online_kpt"]
    k47 = r["pair_index"].index(pairs.index([4, 7]))
    at = [i for i, m in enumerate(s["matches"][pairs.index([4, 7])].tolist()) if m == [where[(4, special["online"])], k7]]
    assert len(at) == 1 and v["keep"][k47][at[0]] and v["errors"][k47][at[0]].max() < 1e-3 * min(v["thresholds"][k47])
    t = _track_of(r, row(f7, k7))
    assert t >= 0 and t == _track_of(r, row(4, where[(4, special["online"])])) and tri["accept"][t]
    e = np.arange(trk["trk_off"][t], trk["trk_off"][t + 1])
    assert not tri["entry_keep"][e][trk["trk_row"][e] == row(f7, k7)].any() and tri["kept"][t] == len(e) - 1 == 3
    assert np.linalg.norm(tri["xyz"][t] - s["xyz"][special["online"]]) < 0.1
    # ---- the chain merges one track across five frames, from neighbour matches only
    rows = [row(f, where[(f, special["chain"])]) for f in range(5)]
    t = _track_of(r, rows[0])
    assert t >= 0 and all(_track_of(r, x) == t for x in rows) and trk["trk_off"][t + 1] - trk["trk_off"][t] == 5 and tri["kept"][t] == 5
    for i, m in enumerate(s["matches"]):
        a, b = pairs[i]
        if abs(a - b) != 1:
            assert [where.get((a, special["chain"])), where.get((b, special["chain"]))] not in m.tolist()
    # ---- a component with two keypoints of one frame keeps the better of them
    f2, k2 = s["special_rows"]["dup_kpt"]
    t = _track_of(r, row(f2, k2))
    e = np.arange(trk["trk_off"][t], trk["trk_off"][t + 1])
    assert t == _track_of(r, row(2, where[(2, special["dup"])])) and (trk["trk_frame"][e] == 2).sum() == 2
    tr = tri["traces"][t]
    assert tr["same_frame"] == 1 and tr["deduped"] == 1 and tri["accept"][t] and tri["kept"][t] == 3
    in2 = e[trk["trk_frame"][e] == 2]
    assert tri["entry_keep"][in2].sum() == 1 and trk["trk_row"][in2][tri["entry_keep"][in2]][0] == row(2, where[(2, special["dup"])])
    # ---- rays that all meet below 1.5 degrees; a point behind one camera
    t = _track_of(r, row(3, where[(3, special["far"])]))
    tr = tri["traces"][t]
    assert tr["L"] == 3 and tr["low_angle"] == 3 and not tri["accept"][t] and tri["best"][t] == -1
    (fa, ka), (fb, kb) = s["special_rows"]["behind"]
    t = _track_of(r, row(fa, ka))
    tr = tri["traces"][t]
    assert t == _track_of(r, row(fb, kb)) and tr["L"] == 2 and tr["bad_depth"] == 1 and not tri["accept"][t]
    # ---- the refit runs everywhere it is reached
    reached = [x for x in tri["traces"] if x["ls_ok"] is not None]
    assert len(reached) >= 300 and all(x["ls_ok"] and all(x["gn_taken"]) and len(x["gn_taken"]) == TR.GN_STEPS for x in reached)
    assert all(x["exhaustive"] for x in tri["traces"])
    ring = TR.run(TR.ring_scene())
    assert sorted(np.diff(ring["tracks"]["trk_off"]).tolist()) == [2, 3, 17, 63, 64, 65] and ring["tri"]["accept"].all()
    assert [x["exhaustive"] for x in ring["tri"]["traces"]] == [x["L"] <= 16 for x in ring["tri"]["traces"]]


def _planted_groups(s, r):
    """Per planted point: its keypoints grouped by the planted matches that were processed (both ends a keypoint of the point)."""
    owner = {int(s["frame_off"][f]) + k: p for (f, p), k in s["where"].items()}
    edges = []
    for i in r["pair_index"]:
        a, b = s["pairs"][i].tolist()
        for m0, m1 in s["matches"][i].tolist():
            u, w = int(s["frame_off"][a]) + m0, int(s["frame_off"][b]) + m1
            if 0 <= m0 < s["frame_off"][a + 1] - s["frame_off"][a] and 0 <= m1 < s["frame_off"][b + 1] - s["frame_off"][b] and \
                    owner.get(u, -1) == owner.get(w, -2):
                edges.append((u, w))
    lab = TR.components(int(s["frame_off"][-1]), np.array(edges).reshape(-1, 2))
    groups = {}
    for x, p in owner.items():
        groups.setdefault((p, int(lab[x])), []).append(x)
    return [(p, sorted(rows)) for (p, _), rows in groups.items() if len(rows) >= 2]


def _bound(s, p, rows, eps: float, premise: bool) -> tuple:
    """The bound on |X - X*| of a point seen by ``rows`` with pixel errors of at most eps per view (see the test's docstring)
    -> (bound, largest angle between two of the views)."""
    frames = np.searchsorted(s["frame_off"], rows, side="right") - 1
    C = s["table"][frames, 12:15]
    theta = max(TR.angle(s["xyz"][p] - C[a], s["xyz"][p] - C[b]) for a in range(len(rows)) for b in range(a + 1, len(rows)))
    z_over_f = max(float(TR.project(s, int(f), s["xyz"][p])[1][0]) / min(PR.unify(int(s["cam_model"][f]), s["cam_params"][f])[:2]) for f in frames)
    dp = (np.sqrt(len(rows)) + 1.0) * eps if premise else MAX_REPROJ + eps
    return 1.25 * z_over_f * dp / np.sin(theta / 2.0), theta


def _check_recovery(s, r, noise):
    """Every group of a planted point's keypoints that the processed matches join, seen under 2 degrees or more, is an accepted
    track within the bound of the planted point.

    The bound, to first order in |D| / Z for D = X - X*: a displacement D moves the projection in view i by at least
    f / Z_i times D's component across ray i, times the distortion's Jacobian and the obliquity, together > 0.8 on these cameras;
    of two rays that meet under theta, D has a component of |D| sin(theta / 2) at least across one.  So
    |D| <= 1.25 (Z / f) dp / sin(theta / 2), with dp the largest distance between the projections of X and X*.  Every view sees X*
    with a residual of eps = sqrt(2) (noise + 2^-14) at most (uniform noise per coordinate plus the float32 rounding of a
    coordinate below 1024), so X*'s cost over n views is n eps^2 at most; the refit's cost is not larger (asserted), hence each of
    its residuals is sqrt(n) eps at most and dp <= (sqrt(n) + 1) eps.  The point with a second detection 0.9 px away is refit with
    that detection among the inliers: for it dp <= max_reproj_error + eps, which every kept entry satisfies by construction."""
    eps = np.sqrt(2.0) * (noise + 2.0 ** -14)
    tri, trk = r["tri"], r["tracks"]
    checked, worst = 0, 0.0
    for p, rows in _planted_groups(s, r):
        premise = p != s["special"]["dup"]
        bound, theta = _bound(s, p, rows, eps, premise)
        if theta < np.deg2rad(2.0):
            assert p == s["special"]["far"]
            continue
        t = _track_of(r, rows[0])
        assert t >= 0 and all(_track_of(r, x) == t for x in rows) and tri["accept"][t], p
        e = np.arange(trk["trk_off"][t], trk["trk_off"][t + 1])
        kept_rows = trk["trk_row"][e][tri["entry_keep"][e]]
        assert set(rows) <= set(kept_rows.tolist()), p
        if premise:
            tk = TR.Track(s, kept_rows, np.searchsorted(s["frame_off"], kept_rows, side="right") - 1)
            cost = lambda X: float(sum(a * a + b * b for a, b in zip(*tk.residual(X)[1:])))
            assert set(rows) == set(kept_rows.tolist()) and cost(tri["xyz"][t]) <= cost(s["xyz"][p]) * (1 + 1e-9) + 1e-12, p
        d = float(np.linalg.norm(tri["xyz"][t] - s["xyz"][p]))
        assert d <= bound, (p, d, bound)
        checked, worst = checked + 1, max(worst, d / bound)
    print(f"noise {noise}: {checked} planted groups recovered, the largest share of the bound used {worst:.3f}")
    return checked


def test_recovery_without_noise(clean):
    assert _check_recovery(*clean, 0.0) >= 280


def test_recovery_with_noise(noisy):
    assert _check_recovery(*noisy, TR.NOISE) >= 280


@pytest.mark.parametrize("which", ["tri", "ring"])
def test_margins_the_gpu_test_relies_on(which, noisy):
    s, r = noisy if which == "tri" else (TR.ring_scene(), TR.run(TR.ring_scene()))
    v = r["verify"]
    for e, th, ok in zip(v["errors"], v["thresholds"], v["in_range"]):
        for c in range(2):
            assert np.all(np.abs(e[ok, c] - th[c]) > 1e-9 * th[c])
    for tr in r["tri"]["traces"]:
        assert all(abs(x - MAX_REPROJ) > 1e-6 for x in tr["reproj"])
        assert all(abs(x - MIN_ANGLE) > 1e-9 for x in tr["angles"])
        hyps = [h for h in tr["hyps"] if h[3] >= 2]
        for n, (_, i, j, cnt, sse) in enumerate(hyps):
            for _, i2, j2, cnt2, sse2 in hyps[n + 1:]:
                if cnt == cnt2 and (i, j) != (i2, j2):      # the same pair drawn twice ties exactly, by construction
                    assert abs(sse - sse2) > 1e-9 * max(sse, sse2), (tr["L"], i, j, i2, j2)
                if (i, j) == (i2, j2):
                    assert cnt == cnt2 and sse == sse2


def test_components_and_tracks_depend_on_the_edge_set_alone(noisy):
    s, r = noisy
    e = r["verify"]["edges"]
    rng = np.random.RandomState(3)
    again = TR.components(int(s["frame_off"][-1]), e[rng.permutation(len(e))][:, ::-1])
    assert np.array_equal(again, r["label"])
    t = r["tracks"]
    assert np.all(np.diff(t["trk_label"]) > 0) and np.all(np.diff(t["trk_off"]) >= 2)
    for a, b, l in zip(t["trk_off"][:-1], t["trk_off"][1:], t["trk_label"]):
        assert t["trk_row"][a] == l and np.all(np.diff(t["trk_row"][a:b]) > 0)
    assert np.array_equal(s["frame_off"][t["trk_frame"]] + t["trk_kpt"], t["trk_row"])


def test_wave_sum_is_the_lane_order():
    x = np.random.RandomState(0).uniform(size=(200, 3)) * 10.0 ** np.random.RandomState(1).randint(-8, 8, size=(200, 1))
    lanes = np.array([x[l::64].cumsum(0)[-1] if len(x[l::64]) else np.zeros(3) for l in range(64)])
    tree = lanes
    while len(tree) > 1:      # the xor butterfly adds lane l and l ^ o: halves fold onto each other
        tree = tree[:len(tree) // 2] + tree[len(tree) // 2:]
    assert np.array_equal(TR.wave_sum(x), tree[0]) and np.allclose(TR.wave_sum(x), x.sum(0), rtol=1e-12)


def test_host_logic_without_a_gpu(noisy):
    from pram_amd._lib import PramHipError
    from pram_amd.localization import formats, mapbuild
    from pram_amd.localization import triangulation as TG
    s, r = noisy
    # ---- pair de-duplication: the first occurrence wins, in either order
    assert TG.unique_pairs([(0, 1), (1, 0), (2, 3), (0, 1), (3, 2), (1, 2)]).tolist() == [0, 2, 5]
    assert TG.unique_pairs(s["pairs"]).tolist() == r["pair_index"]
    # ---- pair_matches under the four name forms
    store = formats.DictStore()
    m0 = np.array([2, -1, 0, -1, 1], dtype=np.int16)
    sc = np.array([0.5, 0.0, 0.25, 0.0, 1.0], dtype=np.float16)
    formats.write_matches(store, formats.names_to_pair("db/a.jpg", "db/b.jpg"), {"matches0": m0, "matching_scores0": sc})
    formats.write_matches(store, formats.names_to_pair("db/d.jpg", "db/c.jpg"), {"matches0": m0, "matching_scores0": sc})
    store.create_dataset(formats.names_to_pair_old("db/e.jpg", "db/f.jpg") + "/matches0", m0)
    store.create_dataset(formats.names_to_pair_old("db/h.jpg", "db/g.jpg") + "/matches0", m0)
    want = np.array([[0, 2], [2, 0], [4, 1]])
    got = TG.pair_matches(store, [("db/a.jpg", "db/b.jpg"), ("db/c.jpg", "db/d.jpg"), ("db/e.jpg", "db/f.jpg"), ("db/g.jpg", "db/h.jpg")])
    for k, reverse in enumerate((False, True, False, True)):
        assert np.array_equal(got[k][0], want[:, ::-1] if reverse else want) and got[k][0].dtype == np.int64
    assert np.array_equal(got[0][1], sc[[0, 2, 4]]) and np.array_equal(got[1][1], sc[[0, 2, 4]]) and got[2][1] is None
    with pytest.raises(ValueError):
        TG.pair_matches(store, [("db/a.jpg", "db/zzz.jpg")])
    # ---- the scene's own store, one pair stored reversed: what comes back is what was written, in the pair list's orientation
    store, held = TR.match_store(s)
    names = [(TR.frame_name(a), TR.frame_name(b)) for a, b in s["pairs"][[i for i, _ in held]].tolist()]
    assert formats.names_to_pair(TR.frame_name(TR.REVERSED_PAIR[1]), TR.frame_name(TR.REVERSED_PAIR[0])) in store
    assert formats.names_to_pair(TR.frame_name(TR.REVERSED_PAIR[0]), TR.frame_name(TR.REVERSED_PAIR[1])) not in store
    for (i, rows), (m, sc) in zip(held, TG.pair_matches(store, names)):
        assert {tuple(x) for x in m.tolist()} == rows and len(m) == len(rows) == len(sc), i
    # ---- unknown parameters and the device
    empty = ([], [], (np.zeros((0, 4)), np.zeros((0, 3))), [], [])
    for call in (lambda: TG.triangulate_map(*empty, "cpu", trails=3), lambda: TG.verify_matches({}, [], [], max_err=1.0),
                 lambda: TG.triangulate_tracks({}, {}, max_error=1.0)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(PramHipError):
        TG.triangulate_map(*empty, "cpu")
    assert set(TG.DEFAULTS) == set(TR.DEFAULTS) and all(TG.DEFAULTS[k] == TR.DEFAULTS[k] for k in TR.DEFAULTS)
    # ---- the tracks dict goes through mapbuild.track_tables as it is
    ids = [100 + f for f in range(s["n_frames"])]
    out = TG.map_tables(ids, s["frame_off"], r["tracks"], r["tri"])
    P = int(r["tri"]["accept"].sum())
    assert out["point_ids"].tolist() == list(range(1, P + 1)) and out["point3D_xyzs"].shape == (P, 3)
    tab = mapbuild.track_tables(SimpleNamespace(frame_ids=ids), out["tracks"])
    keep = r["tri"]["entry_keep"] & np.repeat(r["tri"]["accept"], np.diff(r["tracks"]["trk_off"]))
    assert np.array_equal(tab["point_ids"], out["point_ids"]) and np.array_equal(tab["trk_frame"], r["tracks"]["trk_frame"][keep])
    assert np.array_equal(tab["trk_kpt"], r["tracks"]["trk_kpt"][keep]) and (np.diff(tab["trk_off"]) == r["tri"]["kept"][r["tri"]["accept"]]).all()
    for f, fr in enumerate(out["frames"]):
        assert fr["point3D_ids"].shape == (s["frame_off"][f + 1] - s["frame_off"][f],) and fr["point3D_ids"].dtype == np.int64
        has = fr["point3D_ids"] >= 1
        assert np.array_equal(fr["xyzs"][has], out["point3D_xyzs"][fr["point3D_ids"][has] - 1]) and not fr["xyzs"][~has].any()
    assert sum(int((fr["point3D_ids"] >= 1).sum()) for fr in out["frames"]) == int(keep.sum())
    for word in ("Merge", "Retriangulate", "0.5", "estimation_and_geometric_verification", "database", "dropped"):
        assert word in TG.__doc__, word
