"""GPU: triangulation on the device (pram_amd.localization.triangulation, csrc/triangulate.hip) against the numpy restatement
tests/triangulation_ref.py, stage by stage and end to end, on the planted scene (which special case takes which branch:
tests/test_triangulation_cpu.py, which also asserts the margins that make the discrete results here exact) and on a ring of 70
frames whose tracks have 2, 3, 17, 63, 64 and 65 entries.  profiles/triangulation_parity.md has the measured deviations behind
XYZ_BAR."""
import numpy as np
import pytest
import torch

from tests import pose_ref as PR
from tests import triangulation_ref as TR

pytestmark = pytest.mark.gpu

NORM_BAR = 1e-15      # measured: bit-equal; ten ulps of a normalised coordinate, which is below 1 (the pose stage's bar for the same loop)
# On |X - X_ref| / (1 + |X_ref|) and on the errors in pixels.  Measured: bit-equal on all 328 tracks (the restatement runs the
# kernel's order of operations and the library is built without contraction), and 100 times nothing is nothing; the bar is ten
# ulps of the largest value compared (4 px), far below the 1e-8 it may not exceed.  profiles/triangulation_parity.md.
XYZ_BAR = 1e-14


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


@pytest.fixture(scope="module")
def scenes(TG, dev):
    """Each scene with its restatement (computed once) and its device table."""
    out = {}
    for name, s in (("tri", TR.tri_scene()), ("ring", TR.ring_scene())):
        out[name] = (s, TR.run(s), _table(TG, s, dev))
    return out


def test_frame_table_and_normalisation_all_models(TG, dev):
    """0, 1, 255, 256 and 257 keypoints per frame under each of the five camera models, both pixel offsets."""
    rng = np.random.RandomState(2)
    counts = [c for _ in range(5) for c in (0, 1, 255, 256, 257)]
    cams = [TR.CAMERAS[i // 5] for i in range(25)]
    frames = [{"keypoints": rng.uniform([0, 0], [TR.WIDTH, TR.HEIGHT], size=(n, 2)).astype(np.float32)} for n in counts]
    q = rng.normal(size=(25, 4)) * rng.uniform(0.5, 2.0, size=(25, 1))      # not normalised: the table normalises
    t = rng.normal(size=(25, 3)) * 5.0
    table = TG.frame_table(frames, cams, (q, t), dev)
    rows = [PR.camera_row(c) for c in cams]
    model, params = np.array([r[0] for r in rows]), np.stack([r[1] for r in rows])
    assert table["n_rows"] == sum(counts) and set(model.tolist()) == set(PR.MODELS.values())
    kp = np.concatenate([f["keypoints"] for f in frames])
    for key, off in (("norm0", 0.0), ("norm05", 0.5)):
        want = TR.normalize(kp, table["frame_off_host"], model, params, off)
        got = table[key][:table["n_rows"]].cpu().numpy()
        d = float(np.abs(got - want).max())
        print(f"{key}: largest deviation {d:.3e}")
        assert got.shape == want.shape and d <= NORM_BAR
    want = TR.frame_table(q, t, model, params)
    got = table["frames"].cpu().numpy()
    print(f"frame table: largest deviation / (1 + magnitude) {float((np.abs(got - want) / (1.0 + np.abs(want))).max()):.3e}")
    assert np.all(np.abs(got - want) <= 1e-13 * (1.0 + np.abs(want))) and np.array_equal(got[:, 15], want[:, 15])


def test_verification_equals_the_restatement(TG, scenes):
    s, r, table = scenes["tri"]
    got = TG.verify_matches(table, s["pairs"], s["matches"])
    v = r["verify"]
    assert got["pair_index"].tolist() == r["pair_index"]
    for k in range(len(r["pair_index"])):
        assert np.array_equal(got["keep"][k], v["keep"][k]) and np.array_equal(got["kept"][k], v["kept"][k]), k
    n = np.array([len(k) for k in v["keep"]])
    want = np.where(n > 0, np.array(v["count"]) / np.maximum(n, 1), np.nan)
    assert np.array_equal(got["inlier_ratio"], want, equal_nan=True) and np.isnan(want).sum() == 1
    dropped = sum(int((~ok).sum()) for ok in v["in_range"])
    assert dropped == 3 and all(not k[~ok].any() for k, ok in zip(got["keep"], v["in_range"]))


def test_verification_match_counts(TG, scenes):
    """0, 1, 255, 256 and 257 matches per pair: the pair's planted matches padded with drawn ones, indices out of range among them."""
    s, r, table = scenes["tri"]
    rng = np.random.RandomState(4)
    pairs, matches = [], []
    for (a, b), size in zip(((0, 1), (1, 2), (2, 4), (3, 5), (6, 7)), (0, 1, 255, 256, 257)):
        n0, n1 = (int(s["frame_off"][f + 1] - s["frame_off"][f]) for f in (a, b))
        base = s["matches"][s["pairs"].tolist().index([a, b])]
        drawn = np.stack([rng.randint(-1, n0 + 1, size=size), rng.randint(-1, n1 + 1, size=size)], 1)
        m = np.concatenate([base, drawn])[rng.permutation(len(base) + size)[:size]]
        pairs.append((a, b)); matches.append(m)
    want = TR.verify(s["norm0"], s["frame_off"], s["table"], np.array(pairs), matches)
    for e, th, ok in zip(want["errors"], want["thresholds"], want["in_range"]):      # the margin that makes the mask exact
        assert all(np.all(np.abs(e[ok, c] - th[c]) > 1e-9 * th[c]) for c in range(2))
    got = TG.verify_matches(table, pairs, matches)
    assert [len(k) for k in got["keep"]] == [0, 1, 255, 256, 257]
    for k in range(5):
        assert np.array_equal(got["keep"][k], want["keep"][k]) and np.array_equal(got["kept"][k], want["kept"][k]), k
    assert sum(want["count"]) >= 100 and sum(int((~ok).sum()) for ok in want["in_range"]) >= 3


@pytest.mark.parametrize("name", ["tri", "ring"])
def test_components_and_tracks_equal_the_restatement(TG, scenes, name):
    s, r, table = scenes[name]
    edges = r["verify"]["edges"]
    got = TG.build_tracks(table, edges)
    assert np.array_equal(got["label"], r["label"])
    for k in ("trk_off", "trk_label", "trk_row", "trk_frame", "trk_kpt"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], r["tracks"][k]), k
    if name == "ring":
        assert sorted(np.diff(got["trk_off"]).tolist()) == [2, 3, 17, 63, 64, 65]
    rng = np.random.RandomState(6)
    for _ in range(2):      # the order of the pairs, of a pair's matches and of a match's ends changes no bit
        e = edges[rng.permutation(len(edges))]
        flip = rng.uniform(size=len(e)) < 0.5
        e = np.where(flip[:, None], e[:, ::-1], e)
        again = TG.build_tracks(table, np.concatenate([e, [[-1, 3], [5, int(s["frame_off"][-1])]]]))      # ends outside the table: ignored
        assert all(np.array_equal(again[k], got[k]) for k in got)
    none = TG.build_tracks(table, np.zeros((0, 2), dtype=np.int64))
    assert len(none["trk_off"]) == 1 and none["trk_off"][0] == 0 and np.array_equal(none["label"], np.arange(s["frame_off"][-1]))


def test_one_long_chain_is_one_track(TG, scenes):
    """All rows of the planted scene on one chain, given in descending order: the label of every row is row 0, one track."""
    s, _, table = scenes["tri"]
    n = int(s["frame_off"][-1])
    got = TG.build_tracks(table, np.stack([np.arange(n - 1, 0, -1), np.arange(n - 2, -1, -1)], 1))
    assert not got["label"].any() and got["trk_off"].tolist() == [0, n] and np.array_equal(got["trk_row"], np.arange(n))
    assert np.array_equal(s["frame_off"][got["trk_frame"]] + got["trk_kpt"], got["trk_row"])


@pytest.mark.parametrize("name", ["tri", "ring"])
def test_triangulation_equals_the_restatement(TG, scenes, name):
    s, r, table = scenes[name]
    want = r["tri"]
    got = TG.triangulate_tracks(table, r["tracks"])
    assert np.array_equal(got["accept"], want["accept"]) and np.array_equal(got["best"], want["best"])
    assert np.array_equal(got["kept"], want["kept"]) and np.array_equal(got["entry_keep"], want["entry_keep"])
    assert np.array_equal(got["entry_error"] >= 0, want["entry_error"] >= 0)
    ok = want["best"] >= 0
    dx = np.linalg.norm(got["xyz"][ok] - want["xyz"][ok], axis=1) / (1.0 + np.linalg.norm(want["xyz"][ok], axis=1))
    de, dee = np.abs(got["error"] - want["error"]), np.abs(got["entry_error"] - want["entry_error"])
    print(f"{name}: {int(ok.sum())} tracks, largest |X - X_ref| / (1 + |X_ref|) {dx.max():.3e}, mean error {de.max():.3e} px, entry error {dee.max():.3e} px")
    assert dx.max() <= XYZ_BAR and de.max() <= XYZ_BAR and dee.max() <= XYZ_BAR
    assert not got["xyz"][~ok].any() and not got["entry_keep"][np.repeat(~ok, np.diff(r["tracks"]["trk_off"]))].any()
    if name == "ring":
        assert (np.diff(r["tracks"]["trk_off"]) > 16).sum() == 4 and got["accept"].all()      # four tracks on the sampler's path


def test_seed_and_trials_change_nothing_within_the_exhaustive_budget(TG, scenes):
    s, r, table = scenes["tri"]
    assert np.diff(r["tracks"]["trk_off"]).max() <= 10      # 45 pairs at most
    a = TG.triangulate_tracks(table, r["tracks"])
    b = TG.triangulate_tracks(table, r["tracks"], seed=12345, trials=45)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
    s, r, table = scenes["ring"]      # and beyond it the seed matters only to the tracks that are sampled
    a, b = TG.triangulate_tracks(table, r["tracks"]), TG.triangulate_tracks(table, r["tracks"], seed=12345)
    short = np.diff(r["tracks"]["trk_off"]) <= 16
    assert np.array_equal(a["xyz"][short], b["xyz"][short]) and not np.array_equal(a["best"][~short], b["best"][~short])


def _same(a, b) -> bool:
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def mapped(TG, scenes, dev):
    s = scenes["tri"][0]
    return [TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev) for _ in range(2)]


def test_triangulate_map_is_the_stages_and_repeats_bit_for_bit(TG, scenes, mapped, dev):
    s, r, _ = scenes["tri"]
    assert _same(mapped[0], mapped[1])
    want = TG.map_tables(np.arange(s["n_frames"]), s["frame_off"], r["tracks"], r["tri"])
    m = mapped[0]
    assert np.array_equal(m["point_ids"], want["point_ids"]) and m["point_ids"][0] == 1 and len(m["point_ids"]) == int(r["tri"]["accept"].sum())
    assert _same(m["tracks"], want["tracks"]) and _same([f["point3D_ids"] for f in m["frames"]], [f["point3D_ids"] for f in want["frames"]])
    assert np.abs(m["point3D_xyzs"] - want["point3D_xyzs"]).max() <= XYZ_BAR * (1 + np.abs(want["point3D_xyzs"]).max())
    assert m["pair_index"].tolist() == r["pair_index"] and m["point3D_xyzs"].dtype == np.float64 and m["track_error"].shape == m["point_ids"].shape
    # the pairs and every pair's matches in another order: the same bits
    rng = np.random.RandomState(8)
    order = rng.permutation(r["pair_index"])      # the processed pairs only: which of a repeated pair is met first decides its matches
    shuffled = [s["matches"][i][rng.permutation(len(s["matches"][i]))] for i in order.tolist()]
    again = TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"][order], shuffled, dev)
    for k in ("point_ids", "point3D_xyzs", "track_error", "tracks", "frames"):
        assert _same(again[k], m[k]), k


def test_end_to_end_into_a_reference_store(TG, scenes, mapped, dev):
    from pram_amd.localization import labelling as LB
    from pram_amd.localization import mapbuild as MB
    from pram_amd.localization.candidates import ReferenceStore
    s = scenes["tri"][0]
    m = mapped[0]
    xyz = dict(zip(m["point_ids"].tolist(), m["point3D_xyzs"]))
    lab = LB.label_points(m["tracks"], xyz, 4, dev, min_obs=2)
    landmarks, sids = LB.landmarks_from_labels(lab["id"], lab["label"])
    assert sorted(sids) == m["point_ids"].tolist() and len(landmarks) == 4
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
    assert np.array_equal(store.pt_ids, m["point_ids"])
    assert np.array_equal(store._point_values()["pt_xyz"], m["point3D_xyzs"])
    has = store.point3D_ids >= 1
    assert has.sum() == sum(len(t[0]) for t in m["tracks"].values()) and np.array_equal(store.xyzs[has], m["point3D_xyzs"][store.point3D_ids[has] - 1])
    assert set(out["seg_ref_frame_ids"]) == set(landmarks)


def test_refusals(TG, scenes, dev):
    from pram_amd._lib import PramHipError
    s, r, table = scenes["tri"]
    with pytest.raises(ValueError):
        TG.verify_matches(table, [(0, s["n_frames"])], [np.zeros((0, 2))])
    with pytest.raises(ValueError):
        TG.verify_matches(table, [(0, 1)], [])
    with pytest.raises(TypeError):
        TG.triangulate_map(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), s["pairs"], s["matches"], dev, max_errors=2.0)
    bad = [("FISHEYE", 1, 1, [1.0, 0.0, 0.0])] + list(s["cameras"][1:])
    with pytest.raises(ValueError):
        TG.frame_table(s["frames"], bad, (s["qvec"], s["tvec"]), dev)
    with pytest.raises(PramHipError):
        TG.frame_table(s["frames"], s["cameras"], (s["qvec"], s["tvec"]), "cpu")
    # a caller's own track table may name rows and frames the tables do not hold: such an entry is never an inlier
    trk = {k: v.copy() for k, v in r["tracks"].items()}
    t = int(np.nonzero(r["tri"]["accept"] & (np.diff(trk["trk_off"]) >= 4))[0][0])
    a = trk["trk_off"][t]
    trk["trk_row"][a], trk["trk_frame"][a + 1] = int(s["frame_off"][-1]), s["n_frames"]
    got = TG.triangulate_tracks(table, trk)
    assert not got["entry_keep"][a] and not got["entry_keep"][a + 1] and got["kept"][t] <= r["tri"]["kept"][t] - 2
    others = np.arange(len(r["tri"]["accept"])) != t
    assert np.array_equal(got["accept"][others], r["tri"]["accept"][others])
