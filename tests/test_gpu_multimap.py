"""GPU: several maps behind one store (pram_amd.localization.multimap, pram_cand_plan_maps in csrc/candidates.hip) against the numpy
restatement tests/multimap_ref.py: the plan kernel on hand-built tables, the candidate stages on two maps that share raw point ids
and frame ids, localisation + refinement + tracking on one map stored twice (every query beside its class-shifted twin), a
one-map store against the ReferenceStore it wraps, and the C entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import helpers as H
from tests import multimap_ref as MR
from tests import pose_ref as PR
from tests import refine_ref as RR
from tests import track_ref as TR

pytestmark = pytest.mark.gpu

E2E_Q_BAR, E2E_T_BAR = 1e-8, 2e-8      # DESIGN.md 4.12's bars (tests/test_gpu_pose.py), the same kernels
LOC = dict(seg_k=RR.SEG_K, min_kpts=32, threshold=4.0, min_inliers=30, semantic_matching=False, trials=1000, seed=4)
LISTS = RR.STACK_KEYS


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gml(dev, precision=None):
    from pram_amd.nets.gml import GML
    g = GML({})
    g.load_state_dict(H.gml_sd(), strict=True)
    g.precision = precision
    return g.to(dev).eval()


def _bits(t):
    t = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(t).reshape(-1).view(np.uint8)


def _stores(maps, dev=None, **kw):
    from pram_amd.localization.candidates import ReferenceStore
    return [ReferenceStore(m["frames"], m["seg_ref_frame_ids"], m["start_sid"], device=dev, **kw) for m in maps]


def _multi(maps, names, dev, **kw):
    from pram_amd.localization.multimap import MultiMapStore
    return MultiMapStore(_stores(maps, **kw), names, device=dev)


# ---------------------------------------------------------------- the plan kernel on hand-built tables
def _hand_frame(rng, fid, labels):
    n = len(labels)
    return {"id": fid, "keypoints": rng.uniform(0, 400, (n, 3)).astype(np.float32), "descriptors": CR._unit(rng.standard_normal((n, 128))),
            "xyzs": rng.standard_normal((n, 3)), "point3D_ids": np.arange(n, dtype=np.int64) + 1, "keypoint_segs": np.array(labels, dtype=np.int32),
            "width": 640, "height": 480}


def _hand_maps():
    """Three maps of 2, 1 and 2 frames (300 and 3, 40, 120 and 64 rows) at global landmarks 0 .. 2, 3 .. 4 and 7 .. 10: ids 5 and 6
    are nobody's, landmark 10 (in-map 3 of the last map) has no reference frame."""
    rng = np.random.default_rng(3)
    lab = lambda n, probs: rng.choice(len(probs), n, p=probs).tolist()
    m0 = {"frames": [_hand_frame(rng, 100, lab(300, [0.4, 0.3, 0.3])), _hand_frame(rng, 101, [1, 0, 1])],
          "seg_ref_frame_ids": {0: [100], 1: [101], 2: [100, 101]}, "start_sid": 0}
    m1 = {"frames": [_hand_frame(rng, 100, lab(40, [0.5, 0.5]))], "seg_ref_frame_ids": {0: [100], 1: [100]}, "start_sid": 3}
    m2 = {"frames": [_hand_frame(rng, 100, lab(120, [0.3, 0.1, 0.6])), _hand_frame(rng, 101, [1] * 40 + [3] * 24)],
          "seg_ref_frame_ids": {0: [100], 1: [101], 2: [100], 3: []}, "start_sid": 7}
    return [m0, m1, m2]


HAND_COUNTS = (0, 1, 255, 256, 257, 600)
HAND_N, HAND_CLASSES = 640, 16
# per query: the global labels most of its keypoints carry (the labels of one frame of one map), and its five votes (vote id =
# global landmark + 1): the frame's own landmarks, other maps' (in-map id 0 of maps 1 and 2 among them: 4 and 8), background (0),
# the gap (6, 7), ids past the last map (12 .. 15) and the landmark without a frame (11)
HAND_HOME = ((0, 1, 2), (3, 4), (3, 4), (7, 8, 9), (8, 10), (0, 1, 2))
HAND_VOTES = ((1, 4, 8, 6, 12), (4, 5, 1, 0, 13), (5, 4, 8, 7, 11), (8, 10, 9, 4, 15), (9, 11, 8, 3, 6), (3, 1, 2, 8, 4))
HAND_TOKENS = ((0, 0, 0, 0, 0), (1, 1, 1, 0, 0), (21, 20, 19, 40, 40), (100, 20, 19, 21, 30), (257, 100, 19, 20, 5), (300, 200, 21, 19, 20))
HAND_N_WIN = (0, 4, 5, 5, 4, 5)      # queries 0, 1 and 4: fewer winners than seg_k = 5
HAND_MIN_KPTS = 20


def _hand_votes(dev, seg_k):
    rng = np.random.default_rng(9)
    seg_ids = np.full((len(HAND_COUNTS), HAND_N), -2, dtype=np.int32)
    for b, (nq, home) in enumerate(zip(HAND_COUNTS, HAND_HOME)):
        own = rng.uniform(0, 1, nq) < 0.75
        seg_ids[b, :nq] = np.where(own, rng.choice(home, nq), rng.integers(-1, HAND_CLASSES - 1, nq))
    t = lambda a: torch.tensor(np.asarray(a)[:, :seg_k].copy(), dtype=torch.int32, device=dev)
    n_win = torch.tensor([min(v, seg_k) for v in HAND_N_WIN], dtype=torch.int32, device=dev)
    return {"win_sid": t(HAND_VOTES), "win_count": t(HAND_TOKENS), "n_win": n_win, "seg_ids": torch.from_numpy(seg_ids).to(dev),
            "counts": torch.tensor(HAND_COUNTS, dtype=torch.int32, device=dev), "host_seg_ids": seg_ids}


def _expected_plan(maps, store, votes, seg_k, min_kpts, semantic_matching):
    """Every column of the table from the restatement's decision per (query, vote); -> (plan [10, B * seg_k], the branches met)."""
    B = len(HAND_COUNTS)
    want = np.zeros((10, B * seg_k), dtype=np.int32)
    seen = set()
    n_win = votes["n_win"].cpu().numpy()
    for b, nq in enumerate(HAND_COUNTS):
        for w in range(seg_k):
            p = b * seg_k + w
            live = w < n_win[b]
            gsid = HAND_VOTES[b][w] - 1 if live else -1
            ntok = min(HAND_TOKENS[b][w], nq)
            d = MR.decide(votes["host_seg_ids"][b, :nq], ntok, maps, gsid, min_kpts=min_kpts, semantic_matching=semantic_matching) if live else None
            if d is None:
                want[:, p] = [b, gsid, -1, 0, 0, 0, -1, 0, -1, w]
                seen.add("not live" if not live else "background" if gsid < 0 else "nobody's" if MR.owner(maps, gsid) is None else "no frame")
                continue
            g = int(store.map_frame_off[d["map"]]) + d["frame"]
            frame = maps[d["map"]]["frames"][d["frame"]]
            sem, by = d["semantic_matching"], d["by_sid"]
            rows = CR.frame_rows(frame, d["lsid"] if by else None)
            want[:, p] = [b, gsid, g, int(sem), ntok if sem else nq, len(rows), p * HAND_N if sem else -1, int(store.frame_off[g]),
                          int(store.lm_sel_off[gsid]) if by else -1, w]
            if by:
                assert np.array_equal(store.sel_rows[want[8, p]:want[8, p] + len(rows)], rows + store.frame_off[g])
            seen.add((d["map"], "by sid" if by else "sid 0" if sem else "few tokens" if ntok < min_kpts else "inconsistent"))
    return want, seen


@pytest.fixture(scope="module")
def hand(dev):
    maps = _hand_maps()
    return {"maps": maps, "store": _multi(maps, ["p", "q", "r"], dev)}


@pytest.mark.parametrize("seg_k", [5, 1])
def test_plan_kernel_exact(hand, dev, seg_k):
    """pram_cand_plan_maps against the restatement, column for column: counts 0 .. 600 at n = 640 (the kernel strides by 256), fewer
    winners than seg_k, votes for the background, the gap, ids past the last map, a landmark without a frame and in-map id 0 of
    maps 1 and 2, token counts on both sides of min_kpts, the switch; twice, bit-equal."""
    from pram_amd import ops
    maps, store = hand["maps"], hand["store"]
    assert store.lm_frame.tolist() == [0, 1, 0, 2, 2, -1, -1, 3, 4, 3, -1] and store.lm_start.tolist() == [0, 0, 0, 3, 3, 0, 0, 7, 7, 7, 7]
    assert np.diff(store.frame_off).tolist() == [300, 3, 40, 120, 64]
    v = _hand_votes(dev, seg_k)
    t = store.tables(dev)
    assert "lm_start" in t and t["n_maps"] == 3 and t["start_sid"] == 0
    seen = set()
    for min_kpts, sem in ((HAND_MIN_KPTS, True), (1, True), (HAND_MIN_KPTS, False)):
        run = lambda: ops.cand_plan(v["win_sid"], v["win_count"], v["n_win"], v["seg_ids"], v["counts"], HAND_CLASSES, t, min_kpts, 0.5, sem)
        plan = run()
        want, s = _expected_plan(maps, store, v, seg_k, min_kpts, sem)
        got = plan.cpu().numpy()
        assert np.array_equal(got, want), [(p, got[:, p].tolist(), want[:, p].tolist()) for p in np.nonzero((got != want).any(0))[0]]
        assert torch.equal(run(), plan)
        if sem:
            seen |= s
        else:
            assert not want[3].any()
    if seg_k == 5:
        assert {"not live", "background", "nobody's", "no frame"} <= seen, seen
        for m in range(3):
            assert {(m, "by sid"), (m, "inconsistent"), (m, "few tokens")} <= seen, (m, seen)
        assert {(1, "sid 0"), (2, "sid 0")} <= seen, seen


def test_plan_single_map_equals_pram_cand_plan(dev):
    """Each hand-built map alone: the table of pram_cand_plan_maps over MultiMapStore([map]) is bit-equal to pram_cand_plan's over
    the ReferenceStore with the map's start_sid (0, 3 and 7: the landmark tables move, the plan does not)."""
    from pram_amd import ops
    from pram_amd.localization.multimap import MultiMapStore
    v = _hand_votes(dev, 5)
    live = 0
    for m in _hand_maps():
        one = _stores([m], dev)[0]
        many = MultiMapStore(_stores([m]), ["only"], device=dev)
        args = (v["win_sid"], v["win_count"], v["n_win"], v["seg_ids"], v["counts"], HAND_CLASSES)
        for min_kpts, sem in ((HAND_MIN_KPTS, True), (1, True), (HAND_MIN_KPTS, False)):
            a = ops.cand_plan(*args, one.tables(dev), min_kpts, 0.5, sem)
            b = ops.cand_plan(*args, many.tables(dev), min_kpts, 0.5, sem)
            assert "lm_start" not in one.tables(dev) and torch.equal(a, b), (m["start_sid"], min_kpts, sem)
            live += int((a[2] >= 0).sum())
    assert live > 30


def test_c_entry(hip_lib, hand, dev):
    """pram_cand_plan_maps through ctypes alone: a table equal to the wrapper's, a reference frame at or beyond n_frames rejected as
    an empty pair, batch = 0, and every error status pram_cand_plan's test asks of that entry."""
    from pram_amd import ops
    L = hip_lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    v, t = _hand_votes(dev, 5), hand["store"].tables(dev)
    B, seg_k = len(HAND_COUNTS), 5
    plan = torch.full((10, B * seg_k), -7, dtype=torch.int32, device=dev)

    def run(min_kpts=HAND_MIN_KPTS, n_class=HAND_CLASSES, batch=B, n_frames=t["n_frames"], lm_start=t["lm_start"], plan_=plan, ratio=0.5):
        return L.pram_cand_plan_maps(p(v["win_sid"]), p(v["win_count"]), p(v["n_win"]), p(v["seg_ids"]), p(v["counts"]), batch, HAND_N, n_class, seg_k,
                                     p(t["lm_frame"]), p(t["lm_sel_off"]), p(t["lm_sel_len"]), t["n_landmarks"], p(lm_start), p(t["frame_off"]),
                                     p(t["hist_off"]), p(t["hist_label"]), p(t["hist_cnt"]), n_frames, min_kpts, C.c_double(ratio), 1, p(plan_), st)
    assert run() == 0
    want = ops.cand_plan(v["win_sid"], v["win_count"], v["n_win"], v["seg_ids"], v["counts"], HAND_CLASSES, t, HAND_MIN_KPTS, 0.5, True)
    assert torch.equal(plan, want)
    # the store's frames 3 and 4 (the last map's) are beyond n_frames = 3: their pairs are empty, the others as before
    assert run(n_frames=3) == 0
    got, w = plan.cpu().numpy(), want.cpu().numpy()
    late = w[2] >= 3
    assert late.any() and (got[2][late] == -1).all() and not got[3:6, late].any() and np.array_equal(got[1], w[1]) and np.array_equal(got[:, ~late], w[:, ~late])
    assert (got[6][late] == -1).all() and (got[8][late] == -1).all() and not got[7][late].any()
    plan.fill_(-7)
    assert run(batch=0) == 0
    torch.cuda.synchronize()
    assert (plan == -7).all()
    # error statuses: nothing is launched
    E_ARG = -1
    assert run(min_kpts=-1) == E_ARG and b"min_kpts" in L.pram_last_error() and b"pram_cand_plan_maps" in L.pram_last_error()
    assert run(n_class=2000) == E_ARG
    assert run(ratio=float("nan")) == E_ARG
    assert run(lm_start=None) == E_ARG and b"null" in L.pram_last_error()
    assert run(plan_=plan.view(torch.int8).view(-1)[1:]) == E_ARG and b"misaligned" in L.pram_last_error()
    assert run(batch=70000) == E_ARG
    torch.cuda.synchronize()
    assert (plan == -7).all()


# ---------------------------------------------------------------- two maps sharing raw ids: the candidate stages
@pytest.fixture(scope="module")
def two(dev):
    maps = MR.two_maps()
    qs = MR.pinned_cases(maps)
    feats, seg = CR.batch_features(qs, dev)
    kw = dict(seg_k=MR.TWO_SEG_K, min_kpts=MR.TWO_MIN_KPTS)
    return {"maps": maps, "queries": qs, "store": _multi(maps, MR.TWO_NAMES, dev), "features": feats, "seg": seg, "kw": kw,
            "ref": [MR.candidates(MR.real(q), maps, **kw) for q in qs]}


@pytest.mark.parametrize("precision", ["x3", "f32"])
def test_two_maps_match_candidates(two, dev, precision):
    """mixed_query and one query per map through match_candidates: plan rows exact, the gathered matcher inputs of every pair
    bit-equal to the rows the restatement selects, the lists bit-equal to the restatement fed with the device's matches0 (point
    ids after split_point_ids: the owning map and the raw id), reference_frame_id the (name, id) pair."""
    from pram_amd import ops
    from pram_amd.localization import candidates as cd
    s, store, maps = two, two["store"], two["maps"]
    seg_k = s["kw"]["seg_k"]
    planned = cd.plan_candidates(s["features"], s["seg"], store, **s["kw"])
    plan = dict(zip(ops.CAND_PLAN_FIELDS, planned["plan"].cpu().numpy()))
    data = cd.gather_candidates(s["features"], planned, store)
    host = {k: v.cpu().numpy() for k, v in data.items() if torch.is_tensor(v)}
    out = cd.match_candidates(s["features"], s["seg"], store, _gml(dev, precision), **s["kw"])
    n_matches, per_map = 0, [0, 0]
    for b, ref in enumerate(s["ref"]):
        q = MR.real(s["queries"][b])
        assert len(ref) == seg_k == len(out[b])
        for w, c in enumerate(ref):
            p = b * seg_k + w
            fr = maps[c["map"]]["frames"][c["reference_frame"]]
            got = (plan["query"][p], plan["sid"][p], plan["frame"][p], plan["semantic"][p], plan["lens0"][p], plan["lens1"][p], plan["order"][p])
            want = (b, c["sid"], c["store_frame"], int(c["semantic_matching"]), len(c["q_kpt_ids"]), len(c["ref_rows"]), w)
            assert got == want, (b, w, got, want)
            l0, l1 = len(c["q_kpt_ids"]), len(c["ref_rows"])
            for side, l in (("0", l0), ("1", l1)):
                assert np.array_equal(host["descriptors" + side][p, :l], c["data"]["descriptors" + side]), (b, w, side)
                assert np.array_equal(host["scores" + side][p, :l], c["data"]["scores" + side])
                assert not host["descriptors" + side][p, l:].any() and not host["scores" + side][p, l:].any()
            assert np.array_equal(host["norm_keypoints0"][p, :l0], CR.normalize(c["data"]["keypoints0"], q["width"], q["height"]))
            assert np.array_equal(host["norm_keypoints1"][p, :l1], CR.normalize(c["data"]["keypoints1"], fr["width"], fr["height"]))
            cand = out[b][w]
            assert cand["reference_frame_id"] == (MR.TWO_NAMES[c["map"]], fr["id"]) and cand["sid"] == c["sid"] and cand["order"] == w
            assert cand["semantic_matching"] == c["semantic_matching"] and cand["n_query_kpts"] == l0 and cand["n_ref_kpts"] == l1
            c = dict(c, matches0=cand["matches0"].cpu().numpy())
            lists = CR.correspondences(c, q, fr)
            trimmed = cd.trim_candidate(cand)
            for key, v in lists.items():
                g = trimmed[key].cpu().numpy()
                if key == "matched_point3D_ids":
                    gm, g = store.split_point_ids(g)
                    assert (gm == c["map"]).all()
                assert g.shape == v.shape and np.array_equal(_bits(g), _bits(np.ascontiguousarray(v).astype(g.dtype))), (b, w, key)
            n_matches += len(lists["matched_keypoint_ids"])
            per_map[c["map"]] += len(lists["matched_keypoint_ids"])
    print(f"two maps [{precision}]: {n_matches} matches, per map {per_map}")
    assert min(per_map) > 0
    assert [c["map"] for c in s["ref"][0]] == [0, 1, 0, 1, 0, 1]


def _same_tensors(a, b, what=""):
    """two results of one call: tensors and arrays bit-equal, everything else equal"""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same_tensors(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)) and not (a and isinstance(a[0], str)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tensors(x, y, f"{what}[{i}]")
    elif torch.is_tensor(a) or isinstance(a, np.ndarray):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what
    else:
        assert a == b, (what, a, b)


def test_two_maps_determinism(two, dev):
    from pram_amd.localization import candidates as cd
    net = _gml(dev)
    # the matched_* tensors are padded to n_query_kpts rows; the rows beyond n_matches are not written
    run = lambda: [[cd.trim_candidate(c) for c in r] for r in cd.match_candidates(two["features"], two["seg"], two["store"], net, **two["kw"])]
    a, b = run(), run()
    _same_tensors(a, b, "match_candidates")
    assert sum(int(c["n_matches"]) for r in a for c in r) > 0


# ---------------------------------------------------------------- one map stored twice: every query beside its twin
@pytest.fixture(scope="module")
def twin(dev):
    maps, qs, planted = MR.twin_maps()
    feats, seg = CR.batch_features(qs, dev)
    store = _multi(maps, MR.TWIN_NAMES, dev, covisibility_frame=RR.COVIS)
    return {"maps": maps, "map": maps[0], "queries": qs, "planted": planted, "cams": [p["cam"] for p in planted], "store": store, "features": feats,
            "seg": seg, "graph": RR.covisibility_graph(maps[0], RR.COVIS), "half": len(qs) // 2}


def _check_pose(got, kpts, xyzs, cam, p, what):
    ref = PR.estimate_pose(kpts, xyzs, cam, threshold=LOC["threshold"], trials=LOC["trials"], refine_iters=20, seed=LOC["seed"], p=p)
    assert got["success"] == ref["success"] and got["num_inliers"] == ref["num_inliers"], (what, got["num_inliers"], ref["num_inliers"])
    if not ref["success"]:
        return
    inl = got["inliers"].cpu().numpy() if torch.is_tensor(got["inliers"]) else got["inliers"]
    assert np.array_equal(np.asarray(inl, dtype=bool)[:len(ref["inliers"])], ref["inliers"]), what
    dq = float(np.abs(got["qvec"] - ref["qvec"]).max())
    dt = float(np.abs(got["tvec"] - ref["tvec"]).max() / (1.0 + np.abs(ref["tvec"]).max()))
    print(f"multimap: {what}: inliers {got['num_inliers']}/{len(ref['inliers'])}, dq {dq:.2e} dt {dt:.2e}")
    assert dq <= E2E_Q_BAR and dt <= E2E_T_BAR, (what, dq, dt)


def _same_lists(store, a, b, what, keys=LISTS):
    """the matched lists of a query (map 0) and of its twin (map 1): bit-equal, the point ids after split_point_ids"""
    for k in keys:
        x, y = a[k], b[k]
        if k == "matched_point3D_ids":
            (mx, x), (my, y) = store.split_point_ids(x), store.split_point_ids(y)
            assert bool(((mx == 0) | (x < 0)).all()) and bool(((my == 1) | (y < 0)).all()), (what, "map index")
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (what, k)


def _named(fid, name):
    return fid is None or (isinstance(fid, tuple) and fid[0] == name)


@pytest.mark.parametrize("precision,method", [("x3", "matching"), ("f32", "projection")])
def test_twin_maps_localize_and_refine(twin, dev, precision, method):
    """covisible_scene's map as 'a' and 'b', its five queries followed by their class-shifted twins, through localize_and_refine:
    the twin's candidates go to map b with equal matches0 and bit-equal lists, frames are named a / b throughout (reference frame,
    refinement_reference_frame_ids, slots), covisible slots and frame votes are the one-map restatement's (ids that were not
    scoped would count every point twice), poses equal pose_ref.estimate_pose with the documented pair index inside 4.12's bars,
    and a refined tracked entry with 64 matches or more stands within 1 degree / 0.5 m of its planted camera."""
    from pram_amd import ops
    from pram_amd.localization.refine import localize_and_refine
    s, store, half, seg_k, n_cov = twin, twin["store"], twin["half"], LOC["seg_k"], RR.COVIS
    res = localize_and_refine(s["features"], s["seg"], store, _gml(dev, precision), s["cams"], **LOC, refinement_method=method)
    tables = store.tables(dev)
    methods, n_close = set(), 0
    for b, r in enumerate(res):
        m, name = b // half, MR.TWIN_NAMES[b // half]
        for c in r["candidates"]:
            assert _named(c["reference_frame_id"], name) and (c["reference_frame_id"] is None or c["sid"] // MR.TWIN_START[1] == m), (b, c["sid"])
        if r["success"]:
            kept = r["candidates"][r["order"]]
            n = kept["n_matches_host"]
            _check_pose(r, r["matched_keypoints"].cpu().numpy(), r["matched_xyzs"].cpu().numpy(), s["cams"][b], b * seg_k + r["order"], f"[{precision}] query {b} located")
            assert _named(r["reference_frame_id"], name) and n == len(r["matched_keypoint_ids"])
        x = r["refinement"]
        assert (x is None) == (not r["success"]), b
        if x is None:
            continue
        methods.add(x["method"])
        assert _named(x["reference_frame_id"], name) and all(_named(f, name) for f in x["refinement_reference_frame_ids"])
        _check_pose(x, x["matched_keypoints"].cpu().numpy(), x["matched_xyzs"].cpu().numpy(), s["cams"][b], b, f"[{precision}] query {b} refined by {x['method']}")
        pm, raw = store.split_point_ids(x["matched_point3D_ids"].cpu().numpy())
        assert (pm[raw >= 0] == m).all() and (pm[raw < 0] == -1).all()
        # the frame vote, with its counts, is the ONE map's
        inl = x["inliers"].cpu().numpy()
        votes = RR.find_reference_frames(s["map"], raw[inl] if x["success"] else raw, s["graph"].keys(), with_counts=True)
        assert x["refinement_reference_frame_ids"] == [(name, g) for g, _ in votes[:n_cov]], (b, x["refinement_reference_frame_ids"], votes)
        k = max(1, min(n_cov, store.n_frames))
        cnt = torch.tensor([len(raw)], dtype=torch.int32, device=dev)
        bf, bc, nb = ops.refine_frame_vote(x["matched_point3D_ids"][None].contiguous(), cnt, x["inliers"].to(torch.uint8)[None].contiguous(),
                                           torch.tensor([int(x["success"])], dtype=torch.int32, device=dev), tables, k)
        nb = int(nb[0])
        assert nb == min(k, len(votes)) and bc[0, :nb].tolist() == [c for _, c in votes[:nb]]
        assert [store.frame_ids[i] for i in bf[0, :nb].tolist()] == [(name, g) for g, _ in votes[:nb]]
        if x["method"] == "matching":
            located = {kk: v.cpu().numpy() for kk, v in r.items() if kk.startswith("matched_")}
            located.update(reference_frame_id=r["reference_frame_id"][1], tracking_status=r["tracking_status"], n_slots=n_cov)
            slots = x["slots"]
            stack = RR.refine_stack(MR.real(s["queries"][b]), s["map"], located, lambda d, j: slots[j]["matches0"].cpu().numpy(), s["graph"])
            assert [sl["reference_frame_id"] for sl in slots] == [(name, g) for g in stack["db_ids"]] and x["n_covisible"] == len(stack["db_ids"])
            assert x["used_init"] == stack["used_init"]
            for kk in RR.STACK_KEYS + ("matched_src",):
                g, w = x[kk].cpu().numpy(), np.ascontiguousarray(stack[kk])
                if kk == "matched_point3D_ids":      # the restatement's frames carry raw ids, the localisation's rows store ids
                    g, w = store.split_point_ids(g)[1], store.split_point_ids(w)[1]
                assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w.astype(g.dtype))), (b, kk)
        if r["tracking_status"] and x["success"] and len(raw) >= 64:
            er, ec = PR.pose_errors(PR.qvec_to_rot(x["qvec"]), x["tvec"], s["planted"][b]["R"], s["planted"][b]["t"])
            print(f"multimap [{precision}]: query {b} refined by {x['method']}: {er:.4f} deg, {ec:.4f} m from the planted camera")
            assert er < 1.0 and ec < 0.5
            n_close += 1
    # every query beside its twin
    n_pairs = 0
    for b in range(half):
        a, t = res[b], res[b + half]
        for ca, ct in zip(a["candidates"], t["candidates"]):
            assert ct["sid"] == (ca["sid"] + MR.TWIN_START[1] if ca["sid"] >= 0 else -1) and ca["semantic_matching"] == ct["semantic_matching"]
            assert (ca["reference_frame_id"] is None) == (ct["reference_frame_id"] is None)
            if ca["reference_frame_id"] is not None:
                assert ca["reference_frame_id"] == ("a", ct["reference_frame_id"][1]) and ct["reference_frame_id"][0] == "b"
            assert torch.equal(ca["matches0"], ct["matches0"]) and int(ca["n_matches"]) == int(ct["n_matches"])
            n = int(ca["n_matches"])
            _same_lists(store, {k: ca[k][:n] for k in LISTS}, {k: ct[k][:n] for k in LISTS}, (b, "candidate"))
            n_pairs += ca["reference_frame_id"] is not None
        # the sampler's pair index differs between a query and its twin, so the solver's counts may; its choice may not
        assert (a["success"], a["order"], a["tracking_status"]) == (t["success"], t["order"], t["tracking_status"]), b
        xa, xt = a["refinement"], t["refinement"]
        assert (xa is None) == (xt is None)
        if xa is None:
            continue
        assert xa["method"] == xt["method"]
        _same_lists(store, xa, xt, (b, "refinement"), keys=[k for k in LISTS if k in xa])
        if xa["method"] == "matching":
            assert xa["n_covisible"] == xt["n_covisible"] and torch.equal(xa["matched_src"], xt["matched_src"])
            for sa, st_ in zip(xa["slots"], xt["slots"]):
                assert sa["reference_frame_id"] == ("a", st_["reference_frame_id"][1]) and st_["reference_frame_id"][0] == "b"
                assert torch.equal(sa["matches0"], st_["matches0"]) and int(sa["n_matches"]) == int(st_["n_matches"])
    print(f"multimap [{precision} {method}]: {n_pairs} candidate pairs per half, methods {sorted(methods)}, {n_close} refined entries at their planted camera")
    assert n_pairs >= 6 and n_close >= 4 and methods == ({"matching"} if method == "matching" else {"matching", "projection"})
    assert res[half - 1]["refinement"] is None and res[-1]["refinement"] is None      # the queries without keypoints


N_MAX = 256
TRACK_LOC = dict(LOC, min_inliers=20)      # tests/test_gpu_track.py's arguments for the same scene
REFINE_BELOW = 80


@pytest.fixture(scope="module")
def twin_sequence(dev):
    m, frames, planted = TR.sequence_scene()
    maps = [MR.twin_of(m, s) for s in MR.TWIN_START]
    frames = [MR.twin_queries(row, RR.N_PAD) for row in frames]
    store = _multi(maps, MR.TWIN_NAMES, dev, covisibility_frame=RR.COVIS)
    return {"maps": maps, "map": m, "frames": frames, "planted": [row + row for row in planted], "store": store,
            "steps": [CR.batch_features(row, dev) for row in frames], "graph": RR.covisibility_graph(m, RR.COVIS),
            "index": {fid: i for i, fid in enumerate(store.frame_ids)}}


def _np_lists(d):
    return {k: d[k].cpu().numpy() for k in LISTS if d.get(k) is not None}


def _np_refinement(x):
    if x is None:
        return None
    return dict(_np_lists(x), success=x["success"], num_inliers=x["num_inliers"], inliers=x["inliers"].cpu().numpy(), reference_frame_id=x["reference_frame_id"])


@pytest.mark.parametrize("precision,method", [("x3", "matching"), ("f32", "projection")])
def test_twin_maps_tracker(twin_sequence, dev, precision, method):
    """Three Tracker.run calls on sequence_scene over the map stored twice, eight streams (stream s + 4 is the twin of s): per step
    the tracking lists are bit-equal to track_ref fed with the device's matches0, poses equal pose_ref inside the bars, source, lost,
    reference_frame_id (a (name, id) pair) and the whole state (its point ids are store ids) equal TrackerLoop's; a stream and its
    twin take the same branch with equal matches0 and bit-equal lists in maps 0 and 1."""
    from pram_amd.localization.tracker import Tracker
    s, store = twin_sequence, twin_sequence["store"]
    S = 2 * TR.N_STREAMS
    trk = Tracker(store, _gml(dev, precision), S, N_MAX, **TRACK_LOC, refine_below=REFINE_BELOW, refinement_method=method, covisibility_frame=RR.COVIS)
    loop = TR.TrackerLoop(S, min_inliers=TRACK_LOC["min_inliers"], refine_below=REFINE_BELOW)
    streams = list(range(S))
    sources = []
    for t in range(TR.N_FRAMES):
        feats, seg = s["steps"][t]
        cams = [p["cam"] for p in s["planted"][t]]
        qs = [TR.real(q) for q in s["frames"][t]]
        res = trk.run(feats, seg, cams)
        rest = [b for b in streams if res[b]["source"] in ("relocalize", None)]

        def matcher(b, d):
            return res[b]["tracking"]["matches0"][:qs[b]["count"]].cpu().numpy()

        def solver(b, lists):
            tr = res[b]["tracking"]
            for k in LISTS:
                g, w = tr[k].cpu().numpy(), np.ascontiguousarray(lists[k])
                assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w.astype(g.dtype))), (t, b, k)
            _check_pose(tr, lists["matched_keypoints"], lists["matched_xyzs"], cams[b], b, f"[{precision} {method}] step {t} stream {b} tracked")
            return {"success": tr["success"], "num_inliers": tr["num_inliers"], "inliers": tr["inliers"].cpu().numpy()}

        def refiner(b, frame, located, ret):
            x = res[b]["tracking"]["refinement"]
            assert x is not None and x["method"] == method
            name, m = MR.TWIN_NAMES[b // TR.N_STREAMS], b // TR.N_STREAMS
            assert located["reference_frame_id"][0] == name
            if method == "matching":      # the stack over the covisible frames of the OWNING map
                stack = RR.refine_stack(frame, s["map"], dict(located, reference_frame_id=located["reference_frame_id"][1], n_slots=RR.COVIS),
                                        lambda d, j: x["slots"][j]["matches0"].cpu().numpy(), s["graph"])
                assert x["used_init"] == stack["used_init"] and [sl["reference_frame_id"] for sl in x["slots"]] == [(name, g) for g in stack["db_ids"]]
                for k in RR.STACK_KEYS:
                    g, w = x[k].cpu().numpy(), np.ascontiguousarray(stack[k])
                    if k == "matched_point3D_ids":
                        assert (store.split_point_ids(g)[0][g >= 0] == m).all()
                        g, w = store.split_point_ids(g)[1], store.split_point_ids(w)[1]
                    assert np.array_equal(_bits(g), _bits(w.astype(g.dtype))), (t, b, k)
            _check_pose(x, x["matched_keypoints"].cpu().numpy(), x["matched_xyzs"].cpu().numpy(), cams[b], b, f"[{precision} {method}] step {t} stream {b} refined")
            return _np_refinement(x)

        def relocalizer(i, b, frame):
            assert rest[i] == b
            r = res[b]["localization"]
            if not r["success"]:
                return {"success": False}
            _check_pose(r, r["matched_keypoints"].cpu().numpy(), r["matched_xyzs"].cpu().numpy(), cams[b], i * LOC["seg_k"] + r["order"],
                        f"[{precision} {method}] step {t} stream {b} relocalised")
            return dict(_np_lists(r), success=True, reference_frame_id=r["reference_frame_id"], refinement=_np_refinement(r["refinement"]))

        want = loop.step(qs, streams, matcher, solver, refiner, relocalizer, seg_ids=[q["seg_ids"] for q in qs])
        sources.append([r["source"] for r in res])
        assert sources[-1] == [w["source"] for w in want], (t, sources[-1])
        assert trk.lost.tolist() == loop.lost
        for b in streams:
            name = MR.TWIN_NAMES[b // TR.N_STREAMS]
            assert res[b]["success"] == want[b]["success"]
            if not res[b]["success"]:
                continue
            assert res[b]["reference_frame_id"] == want[b]["reference_frame_id"] == trk.reference_frame_id[b] and res[b]["reference_frame_id"][0] == name
            pm, raw = store.split_point_ids(res[b]["matched_point3D_ids"].cpu().numpy())
            assert (pm[raw >= 0] == b // TR.N_STREAMS).all()
            if res[b]["source"] != "relocalize" and len(raw) >= 64:
                p = s["planted"][t][b]
                er, ec = PR.pose_errors(PR.qvec_to_rot(res[b]["qvec"]), res[b]["tvec"], p["R"], p["t"])
                assert er < 1.0 and ec < 0.5, (t, b, er, ec)
        # the whole state
        exp = TR.state_arrays(loop, N_MAX, s["index"])
        got = {k: getattr(trk.state, k).cpu().numpy() for k in ("keypoints", "scores", "descriptors", "counts", "xyzs", "point3D_ids", "seg_ids", "ref_frame", "frame_norm")}
        for st_ in streams:
            n = int(exp["counts"][st_])
            assert got["counts"][st_] == n and got["ref_frame"][st_] == exp["ref_frame"][st_] and np.array_equal(got["frame_norm"][st_], exp["frame_norm"][st_]), (t, st_)
            for k in ("keypoints", "scores", "descriptors"):
                assert np.array_equal(_bits(got[k][st_, :n]), _bits(exp[k][st_, :n])), (t, st_, k)
            for k in ("xyzs", "point3D_ids", "seg_ids"):
                assert np.array_equal(_bits(got[k][st_]), _bits(exp[k][st_])), (t, st_, k)
            ids = got["point3D_ids"][st_]
            assert (store.split_point_ids(ids)[0][ids >= 0] == st_ // TR.N_STREAMS).all()
            if exp["ref_frame"][st_] >= 0:
                assert store.frame_map[exp["ref_frame"][st_]] == st_ // TR.N_STREAMS
        # a stream and its twin
        for b in range(TR.N_STREAMS):
            a, tw = res[b], res[b + TR.N_STREAMS]
            assert a["source"] == tw["source"] and a["success"] == tw["success"]
            if a["tracking"] is not None:
                assert torch.equal(a["tracking"]["matches0"][:qs[b]["count"]], tw["tracking"]["matches0"][:qs[b]["count"]])
                _same_lists(store, a["tracking"], tw["tracking"], (t, b, "tracking"))
            if a["success"]:
                assert a["reference_frame_id"] == ("a", tw["reference_frame_id"][1]) and tw["reference_frame_id"][0] == "b"
                _same_lists(store, a, tw, (t, b, "result"), keys=[k for k in LISTS if a.get(k) is not None])
        print(f"multimap track [{precision} {method}]: step {t}: sources {sources[-1]}, inliers {[r['num_inliers'] for r in res]}")
    flat = [x for row in sources for x in row]
    assert "track" in flat and "track+refine" in flat and "relocalize" in flat
    assert all(row[3] is None and row[7] is None for row in sources)      # the streams without keypoints


# ---------------------------------------------------------------- a one-map store against the store it wraps
def _same_but_names(a, b, name, what=""):
    """a: a result over MultiMapStore([A], [name]); b: the same call over A.  Tensors bit-equal, scalars equal, and wherever b has a
    frame id a has (name, that id)."""
    if isinstance(b, dict):
        assert a.keys() == b.keys(), what
        for k in b:
            if k == "reference_frame_id" or k == "refinement_reference_frame_ids":
                ids_a, ids_b = (a[k], b[k]) if isinstance(b[k], list) else ([a[k]], [b[k]])
                assert ids_a == [None if f is None else (name, f) for f in ids_b], (what, k, ids_a, ids_b)
            else:
                _same_but_names(a[k], b[k], name, f"{what}.{k}")
    elif isinstance(b, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_but_names(x, y, name, f"{what}[{i}]")
    elif torch.is_tensor(b) or isinstance(b, np.ndarray):
        assert type(a) is type(b) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what
    else:
        assert a == b and type(a) is type(b), (what, a, b)


def _written(x, nq=None):
    """A result without the rows no kernel writes: a candidate's matched_* lists and inliers are padded to its n_query_kpts rows
    (the first n_matches are valid), a tracking result's matches0 / scores to the matcher's padded width (the query's count are)."""
    if isinstance(x, list):
        return [_written(v, nq) for v in x]
    if not isinstance(x, dict):
        return x
    out = {k: _written(v, nq) for k, v in x.items()}
    if "n_matches" in x and "matched_keypoints" in x:
        n = int(x["n_matches"])
        out.update({k: v[:n] for k, v in x.items() if k.startswith("matched_") or (k == "inliers" and torch.is_tensor(v))})
    if "tracked" in x and nq is not None:
        out.update({k: x[k][:nq] for k in ("matches0", "matching_scores0")})
    return out


@pytest.mark.parametrize("method", ["matching", "projection"])
def test_single_map_store_equals_reference_store(dev, method):
    """MultiMapStore([A]) against ReferenceStore(A) on covisible_scene, the same batch and the same calls (localize_and_refine, then
    three Tracker.run calls on sequence_scene): every output tensor bit-equal, every scalar equal, frame ids differing by the name."""
    from pram_amd.localization.multimap import MultiMapStore
    from pram_amd.localization.refine import localize_and_refine
    from pram_amd.localization.tracker import Tracker
    m, qs, planted = RR.covisible_scene()
    A = _stores([m], dev, covisibility_frame=RR.COVIS)[0]
    M = MultiMapStore(_stores([m], covisibility_frame=RR.COVIS), ["only"], device=dev)
    feats, seg = CR.batch_features(qs, dev)
    cams = [p["cam"] for p in planted]
    net = _gml(dev)
    one = localize_and_refine(feats, seg, A, net, cams, **LOC, refinement_method=method)
    many = localize_and_refine(feats, seg, M, net, cams, **LOC, refinement_method=method)
    _same_but_names(_written(many), _written(one), "only", "localize_and_refine")
    assert sum(r["refinement"] is not None for r in one) >= 3
    _, frames, tplanted = TR.sequence_scene()
    kw = dict(TRACK_LOC, refine_below=REFINE_BELOW, refinement_method=method, covisibility_frame=RR.COVIS)
    ta, tm = Tracker(A, net, TR.N_STREAMS, N_MAX, **kw), Tracker(M, net, TR.N_STREAMS, N_MAX, **kw)
    for t in range(TR.N_FRAMES):
        f, sg = CR.batch_features(frames[t], dev)
        c = [p["cam"] for p in tplanted[t]]
        rm, ra = tm.run(f, sg, c), ta.run(f, sg, c)
        for b, q in enumerate(frames[t]):
            _same_but_names(_written(rm[b], q["count"]), _written(ra[b], q["count"]), "only", f"run {t} stream {b}")
        for k in ("keypoints", "scores", "descriptors", "counts", "xyzs", "point3D_ids", "seg_ids", "ref_frame", "frame_norm"):
            assert torch.equal(getattr(tm.state, k), getattr(ta.state, k)), (t, k)
        assert tm.lost.tolist() == ta.lost.tolist()
