"""GPU: tracking the last frame for a batch of streams (pram_amd.localization.tracker, csrc/track.hip) against the numpy
restatement tests/track_ref.py: the four kernels on their own, the public calls step by step on sequence_scene, and the C
entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import helpers as H
from tests import pose_ref as PR
from tests import refine_ref as RR
from tests import track_ref as TR

pytestmark = pytest.mark.gpu

E2E_Q_BAR, E2E_T_BAR = 1e-8, 2e-8      # the bars of tests/test_gpu_pose.py for the same kernels
COR_KEYS = ("matched_keypoint_ids", "matched_keypoints", "matched_ref_keypoints", "matched_point3D_ids", "matched_xyzs", "matched_sids")
COR_DTYPES = (torch.int64, torch.float32, torch.float32, torch.int64, torch.float64, torch.int32)
COR_TAILS = ((), (2,), (2,), (), (3,), ())
STATE_KEYS = ("keypoints", "scores", "descriptors", "counts", "xyzs", "point3D_ids", "seg_ids", "ref_frame", "frame_norm")


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    t = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(t).reshape(-1).view(np.uint8)


def _random_bytes(rng, shape, dt, dev):
    """Random bits in 32-bit words, none of which reads as a float32 infinity or NaN: the buffers go back to the caching allocator,
    and what a later test reads from memory it never wrote should at least be finite."""
    words = rng.integers(0, 2 ** 32, int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size() // 4, dtype=np.uint32)
    words[(words & 0x7F800000) == 0x7F800000] &= np.uint32(0xFF7FFFFF)
    return torch.from_numpy(words.view(np.uint8)).view(dt).reshape(shape).to(dev)


def _random_state(rng, S, n_max, dev, counts, p_bare=0.3):
    """A TrackState with random bits in every float (xyz: random 64-bit words), point ids >= 0 except a share p_bare of -1."""
    from pram_amd.localization.tracker import TrackState
    st = TrackState(S, n_max, dev)
    st.keypoints, st.scores, st.descriptors = (_random_bytes(rng, tuple(getattr(st, k).shape), torch.float32, dev) for k in ("keypoints", "scores", "descriptors"))
    st.xyzs = _random_bytes(rng, (S, n_max, 3), torch.float64, dev)
    p3d = rng.integers(0, 2 ** 22, (S, n_max))
    p3d[rng.uniform(0, 1, (S, n_max)) < p_bare] = -1
    st.point3D_ids = torch.from_numpy(p3d).to(dev)
    st.seg_ids = torch.from_numpy(rng.integers(-1, 500, (S, n_max)).astype(np.int32)).to(dev)
    st.counts = torch.tensor(counts, dtype=torch.int32, device=dev)
    st.ref_frame = torch.from_numpy(rng.integers(0, 50, S).astype(np.int32)).to(dev)
    st.frame_norm = torch.from_numpy(rng.uniform(1, 400, (S, 3)).astype(np.float32)).to(dev)
    return st


def _host(st):
    return {k: getattr(st, k).cpu().numpy().copy() for k in STATE_KEYS}


def _sentinel_cor(P, cap, dev):
    out = {k: torch.from_numpy(np.full(int(np.prod((P, cap) + tail)) * torch.empty(0, dtype=dt).element_size(), 0xA5, np.uint8)).view(dt)
           .reshape((P, cap) + tail).to(dev) for k, dt, tail in zip(COR_KEYS, COR_DTYPES, COR_TAILS)}
    out["count"] = torch.full((P,), -7, dtype=torch.int32, device=dev)
    return out


@pytest.mark.parametrize("B", [0, 1, 5])
def test_track_plan_exact(dev, B):
    from pram_amd import ops
    rng = np.random.default_rng(3 + B)
    S, n_max, N = 6, 100, 80
    st = _random_state(rng, S, n_max, dev, [0, 100, 37, 1, 99, 64])
    slots = [[], [4], [-1, 3, 0, 5, -1]][(0, 1, 5).index(B)]
    counts = rng.integers(0, N + 1, B).astype(np.int32)
    if B == 5:
        counts[1], counts[2] = 0, N
    plan, loc = ops.track_plan(torch.from_numpy(counts).to(dev), torch.tensor(slots, dtype=torch.int32, device=dev), st.arrays(), N)
    assert tuple(plan.shape) == (ops.CAND_PLAN_COLS, B) and tuple(loc.shape) == (ops.CAND_PLAN_COLS, B)
    h = _host(st)
    want, want_loc = np.zeros((10, B), np.int32), np.zeros((10, B), np.int32)
    for b, s in enumerate(slots):
        live = s >= 0
        row = [b, -1, s if live else -1, 0, counts[b] if live else 0, h["counts"][s] if live else 0, -1, s * n_max if live else 0, -1, 0]
        want[:, b] = row
        row[2] = h["ref_frame"][s] if live else -1
        want_loc[:, b] = row
    assert np.array_equal(plan.cpu().numpy(), want) and np.array_equal(loc.cpu().numpy(), want_loc)


def _expected_correspond(h, n_max, slot, lens0, lens1, m0, q_kpts, b, cap):
    rows = []
    for i in range(lens0):
        j = int(m0[i])
        if 0 <= j < lens1 and h["point3D_ids"][slot, j] >= 0:
            rows.append((i, j))
    rows = rows[:cap]
    i = np.array([r[0] for r in rows], dtype=np.int64)
    j = np.array([r[1] for r in rows], dtype=np.int64)
    return {"matched_keypoint_ids": i, "matched_keypoints": q_kpts[b, i], "matched_ref_keypoints": h["keypoints"][slot, j],
            "matched_point3D_ids": h["point3D_ids"][slot, j], "matched_xyzs": h["xyzs"][slot, j], "matched_sids": h["seg_ids"][slot, j]}


@pytest.mark.parametrize("cap", [600, 100])
def test_track_correspond_exact(dev, cap):
    """Every lens0 at and around the workgroup's chunk of 256 and the wave's 64; matches of -1, match indices >= lens1, rows
    whose point id is -1, a query without a slot, cap below the count; xyz compared as bits; rows beyond the count untouched."""
    from pram_amd import ops
    rng = np.random.default_rng(17)
    lens0 = [0, 1, 63, 64, 65, 255, 256, 257, 600, 300]
    B, N, S, n_max = len(lens0), 600, 10, 640
    slot = [7, 2, 9, 0, 4, 1, 8, 3, 6, -1]
    st_counts = [640, 0, 500, 1, 64, 257, 640, 333, 65, 128]
    st = _random_state(rng, S, n_max, dev, st_counts)
    h = _host(st)
    counts = torch.tensor(lens0, dtype=torch.int32, device=dev)
    q_kpts = _random_bytes(rng, (B, N, 2), torch.float32, dev)
    plan, _ = ops.track_plan(counts, torch.tensor(slot, dtype=torch.int32, device=dev), st.arrays(), N)
    T = 640
    m0 = np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        l1 = st_counts[slot[b]] if slot[b] >= 0 else 0
        m0[b, :N] = rng.integers(-1, l1 + 6, N)      # -1, and up to five indices at and beyond lens1
        m0[b, rng.uniform(0, 1, T) < 0.2] = -1
    out = ops.track_correspond(torch.from_numpy(m0).to(dev)[:, :N], plan, st.arrays(), q_kpts, cap, out=_sentinel_cor(B, cap, dev))
    sentinel = _sentinel_cor(B, cap, dev)
    got_counts = out["count"].cpu().numpy()
    qk = q_kpts.cpu().numpy()
    dropped = capped = 0
    for b in range(B):
        live = slot[b] >= 0
        want = _expected_correspond(h, n_max, slot[b], lens0[b] if live else 0, st_counts[slot[b]] if live else 0, m0[b], qk, b, cap)
        full = _expected_correspond(h, n_max, slot[b], lens0[b] if live else 0, st_counts[slot[b]] if live else 0, m0[b], qk, b, 10 ** 9)
        n = len(want["matched_keypoint_ids"])
        capped += len(full["matched_keypoint_ids"]) > n
        dropped += live and ((m0[b, :lens0[b]] >= 0).sum() > len(full["matched_keypoint_ids"]))
        assert got_counts[b] == n, (b, got_counts[b], n)
        for k in COR_KEYS:
            assert np.array_equal(_bits(out[k][b, :n]), _bits(want[k])), (b, k)
            assert np.array_equal(_bits(out[k][b, n:]), _bits(sentinel[k][b, n:])), (b, k, "rows beyond the count were written")
    assert got_counts[0] == 0 and got_counts[9] == 0 and dropped >= 4 and (capped >= 2) == (cap == 100)


@pytest.mark.parametrize("mask_kind", ["none", "all", "alternating"])
def test_track_filter_exact(dev, mask_kind):
    from pram_amd import ops
    rng = np.random.default_rng(23)
    counts = [0, 1, 64, 65, 257]
    B, cap = len(counts), 257
    cor = {k: _random_bytes(rng, (B, cap) + tail, dt, dev) for k, dt, tail in zip(COR_KEYS, COR_DTYPES, COR_TAILS)}
    cor["count"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    mask = {"none": np.zeros((B, cap), np.uint8), "all": np.full((B, cap), 0x7F, np.uint8), "alternating": (np.arange(B * cap).reshape(B, cap) % 2).astype(np.uint8)}[mask_kind]
    out = ops.track_filter(cor, torch.from_numpy(mask).to(dev), out=_sentinel_cor(B, cap, dev))
    sentinel = _sentinel_cor(B, cap, dev)
    for b in range(B):
        keep = np.nonzero(mask[b, :counts[b]])[0]
        assert int(out["count"][b]) == len(keep), (b, mask_kind)
        for k in COR_KEYS:
            assert np.array_equal(_bits(out[k][b, :len(keep)]), _bits(cor[k][b].cpu().numpy()[keep])), (b, k)
            assert np.array_equal(_bits(out[k][b, len(keep):]), _bits(sentinel[k][b, len(keep):])), (b, k)
    again = ops.track_filter(cor, torch.from_numpy(mask).to(dev))
    assert torch.equal(again["count"], out["count"])


@pytest.mark.parametrize("N", [1, 64, 65, 192])
@pytest.mark.parametrize("with_mask,with_segs", [(False, True), (True, False)])
def test_track_commit_exact(dev, N, with_mask, with_segs):
    """The state after the commit against initialize_localization_variables + update_point3ds: counts 0 and N, lists with repeated
    keypoint ids (the last row wins), ids out of range, mask NULL and not, seg_ids NULL and not, slots -1 and permuted; slots
    nobody names are bit-equal to before; run twice from the same state, the results are bit-equal."""
    from pram_amd import ops
    rng = np.random.default_rng(31 + N)
    S, n_max, B, cap = 6, 200, 5, 3 * N + 7
    slot = [-1, 4, 0, 2, -1]
    counts = [N, N, 0, max(N // 2, 1), 0]
    q = {"keypoints": _random_bytes(rng, (B, N, 2), torch.float32, dev), "scores": _random_bytes(rng, (B, N), torch.float32, dev),
         "descriptors": _random_bytes(rng, (B, N, 128), torch.float32, dev)}
    seg = torch.from_numpy(rng.integers(-1, 300, (B, N)).astype(np.int32)).to(dev) if with_segs else None
    cor = {"matched_keypoint_ids": torch.from_numpy(rng.integers(-2, N + 2, (B, cap))).to(dev),      # repeats, and ids out of range
           "matched_point3D_ids": torch.from_numpy(rng.integers(0, 2 ** 22, (B, cap))).to(dev),
           "matched_xyzs": _random_bytes(rng, (B, cap, 3), torch.float64, dev),
           "matched_sids": torch.from_numpy(rng.integers(0, 300, (B, cap)).astype(np.int32)).to(dev),
           "count": torch.tensor([cap, cap, cap, cap - 5, 3], dtype=torch.int32, device=dev)}
    mask = torch.from_numpy((rng.uniform(0, 1, (B, cap)) < 0.6).astype(np.uint8)).to(dev) if with_mask else None
    ref = torch.tensor([11, 12, 13, 14, 15], dtype=torch.int32, device=dev)
    norm = (319.5, 239.5, 448.0)
    results = []
    for _ in range(2):
        st = _random_state(np.random.default_rng(5), S, n_max, dev, [200, 17, 0, 64, 100, 1])
        before = _host(st)
        ops.track_commit(st.arrays(), q["keypoints"], q["scores"], q["descriptors"], torch.tensor(counts, dtype=torch.int32, device=dev), seg,
                         torch.tensor(slot, dtype=torch.int32, device=dev), slot, ref, norm, cor, mask)
        results.append(_host(st))
    after = results[0]
    for k in STATE_KEYS:
        assert np.array_equal(_bits(results[0][k]), _bits(results[1][k])), (k, "two runs differ")
    hq = {k: v.cpu().numpy() for k, v in q.items()}
    hc = {k: v.cpu().numpy() for k, v in cor.items()}
    repeats = 0
    for s in range(S):
        if s not in slot:
            for k in STATE_KEYS:
                assert np.array_equal(_bits(after[k][s]), _bits(before[k][s])), (s, k, "a slot nobody names was touched")
            continue
        b = slot.index(s)
        n = counts[b]
        frame = TR.initialize_localization_variables({"keypoints": hq["keypoints"][b, :n]}, seg.cpu().numpy()[b] if with_segs else None)
        m = int(hc["count"][b])
        rows = np.arange(m)
        ids = hc["matched_keypoint_ids"][b, :m]
        ok = (ids >= 0) & (ids < n) & ((mask.cpu().numpy()[b, :m] != 0) if with_mask else True)
        rows = rows[ok]
        repeats += len(rows) - len(np.unique(ids[rows]))
        TR.update_point3ds(frame, {"matched_keypoint_ids": ids[rows], "matched_xyzs": hc["matched_xyzs"][b, rows], "matched_sids": hc["matched_sids"][b, rows],
                                   "matched_point3D_ids": hc["matched_point3D_ids"][b, rows]})
        assert after["counts"][s] == n and after["ref_frame"][s] == int(ref[b]) and after["frame_norm"][s].tolist() == [np.float32(v) for v in norm]
        for k in ("keypoints", "scores", "descriptors"):
            assert np.array_equal(_bits(after[k][s, :n]), _bits(hq[k][b, :n])), (s, k)
            assert np.array_equal(_bits(after[k][s, n:]), _bits(before[k][s, n:])), (s, k, "rows beyond the count were written")
        assert np.array_equal(_bits(after["xyzs"][s, :n]), _bits(frame["xyzs"])) and not after["xyzs"][s, n:].view(np.uint64).any()
        assert np.array_equal(after["point3D_ids"][s, :n], frame["point3D_ids"]) and (after["point3D_ids"][s, n:] == -1).all()
        assert np.array_equal(after["seg_ids"][s, :n], frame["seg_ids"]) and (after["seg_ids"][s, n:] == -1).all()
    assert repeats > 0 or N == 1


# ---------------------------------------------------------------- the public calls
LOC = dict(seg_k=RR.SEG_K, min_kpts=32, threshold=4.0, min_inliers=20, semantic_matching=False, trials=1000, seed=4)
REFINE_BELOW = 80      # between what the narrow streams and the wide one can reach (56 / 44 and 106 points): test arguments, not tolerances
N_MAX = 256


def _gml(dev, precision=None):
    from pram_amd.nets.gml import GML
    g = GML({})
    g.load_state_dict(H.gml_sd(), strict=True)
    g.precision = precision
    return g.to(dev).eval()


def _adagml(dev):
    from pram_amd.nets.adagml import AdaGML
    a = AdaGML({})
    a.load_state_dict(H.adagml_sd(), strict=True)
    return a.to(dev).eval()


@pytest.fixture(scope="module")
def scene(dev):
    from pram_amd.localization.candidates import ReferenceStore
    m, frames, planted = TR.sequence_scene()
    store = ReferenceStore(m["frames"], m["seg_ref_frame_ids"], m["start_sid"], device=dev, covisibility_frame=RR.COVIS)
    steps = [CR.batch_features(frames[t], dev) for t in range(TR.N_FRAMES)]
    return {"map": m, "frames": frames, "planted": planted, "store": store, "steps": steps, "graph": RR.covisibility_graph(m, RR.COVIS),
            "index": {fid: i for i, fid in enumerate(RR.frame_ids(m))}}


def _tracker(scene, net, method="matching", **kw):
    from pram_amd.localization.tracker import Tracker
    args = dict(LOC, refine_below=REFINE_BELOW, refinement_method=method, covisibility_frame=RR.COVIS)
    args.update(kw)
    return Tracker(scene["store"], net, TR.N_STREAMS, N_MAX, **args)


def _alone(net, data, p, l0, l1):
    one = {}
    for side, l in (("0", l0), ("1", l1)):
        for key in ("descriptors", "norm_keypoints", "scores"):
            one[key + side] = data[key + side][p:p + 1, :l].contiguous()
        one["keypoints" + side] = one["norm_keypoints" + side]
    return net.produce_matches(one)


def _tracking_inputs(trk, feats):
    """the grouped call's inputs, rebuilt outside the public call from the state as it stands: for the pairs run alone"""
    from pram_amd import ops
    from pram_amd.localization import candidates as cd
    st = trk.state.arrays()
    B, N = feats["counts"].numel(), feats["keypoints"].shape[1]
    slot = torch.tensor([s if not trk.lost[s] else -1 for s in range(B)], dtype=torch.int32, device=feats["counts"].device)
    plan, _ = ops.track_plan(feats["counts"], slot, st, N)
    dummy = torch.zeros(1, dtype=torch.int32, device=slot.device)
    T = cd.padded_size(N, trk.n_max)
    data = ops.cand_gather(plan, dummy, ops.track_gather_tables(st, dummy), feats["descriptors"], feats["keypoints"], feats["scores"], cd._query_norm(feats), T)
    return data, plan.cpu().numpy()


def _np_lists(d):
    return {k: d[k].cpu().numpy() for k in TR.LIST_KEYS if d.get(k) is not None}


def _np_refinement(x):
    if x is None:
        return None
    return dict(_np_lists(x), success=x["success"], num_inliers=x["num_inliers"], inliers=x["inliers"].cpu().numpy(), reference_frame_id=x["reference_frame_id"])


def _check_pose(got, lists, cam, p, what):
    ref = PR.estimate_pose(lists["matched_keypoints"], lists["matched_xyzs"], cam, threshold=LOC["threshold"], trials=LOC["trials"], refine_iters=20,
                           seed=LOC["seed"], p=p)
    assert got["success"] == ref["success"] and got["num_inliers"] == ref["num_inliers"], (what, got["num_inliers"], ref["num_inliers"])
    if not ref["success"]:
        return
    inl = got["inliers"].cpu().numpy() if torch.is_tensor(got["inliers"]) else got["inliers"]
    assert np.array_equal(np.asarray(inl, dtype=bool)[:len(ref["inliers"])], ref["inliers"]), what
    dq = float(np.abs(got["qvec"] - ref["qvec"]).max())
    dt = float(np.abs(got["tvec"] - ref["tvec"]).max() / (1.0 + np.abs(ref["tvec"]).max()))
    print(f"track: {what}: inliers {got['num_inliers']}/{len(ref['inliers'])}, dq {dq:.2e} dt {dt:.2e}")
    assert dq <= E2E_Q_BAR and dt <= E2E_T_BAR, (what, dq, dt)


def _run_sequence(scene, net, method, tag, check_alone=True):
    """Three run calls; after each, every check of the module docstring's list.  -> the sources per step."""
    from pram_amd.localization.refine import localize_and_refine
    trk = _tracker(scene, net, method)
    loop = TR.TrackerLoop(TR.N_STREAMS, min_inliers=LOC["min_inliers"], refine_below=REFINE_BELOW)
    streams = list(range(TR.N_STREAMS))
    sources = []
    for t in range(TR.N_FRAMES):
        feats, seg = scene["steps"][t]
        cams = [p["cam"] for p in scene["planted"][t]]
        qs = [TR.real(q) for q in scene["frames"][t]]
        was_lost = trk.lost.copy()
        data, plan_host = _tracking_inputs(trk, feats)
        res = trk.run(feats, seg, cams)
        tried = [b for b in streams if not was_lost[b]]
        assert [b for b in streams if res[b]["tracking"] is not None] == tried
        rest = [b for b in streams if res[b]["source"] in ("relocalize", None)]
        # relocalize's result equals localize_and_refine on the same sub-batch, bit for bit
        if rest:
            idx = torch.tensor(rest, device=feats["counts"].device)
            sub = {"keypoints": feats["keypoints"][idx].contiguous(), "scores": feats["scores"][idx].contiguous(), "descriptors": feats["descriptors"][idx].contiguous(),
                   "counts": feats["counts"][idx].contiguous(), "image_size": feats["image_size"]}
            direct = localize_and_refine(sub, seg[idx].contiguous(), scene["store"], net, [cams[b] for b in rest], **LOC, covisibility_frame=RR.COVIS,
                                         refinement_method=method)
            for i, b in enumerate(rest):
                got, want = res[b]["localization"], direct[i]
                assert got["success"] == want["success"] and got["num_inliers"] == want["num_inliers"] and got["reference_frame_id"] == want["reference_frame_id"]
                if want["success"]:
                    assert np.array_equal(got["qvec"], want["qvec"]) and np.array_equal(got["tvec"], want["tvec"]) and torch.equal(got["inliers"], want["inliers"])
                    for k in TR.LIST_KEYS:
                        assert torch.equal(got[k], want[k]), (b, k)
                    _check_pose(got, _np_lists(got), cams[b], i * LOC["seg_k"] + got["order"], f"[{tag}] step {t} stream {b} relocalised")
                xg, xw = got["refinement"], want["refinement"]
                assert (xg is None) == (xw is None)
                if xg is not None:
                    assert xg["success"] == xw["success"] and np.array_equal(xg["qvec"], xw["qvec"]) and torch.equal(xg["matched_xyzs"], xw["matched_xyzs"])
                    assert torch.equal(xg["inliers"], xw["inliers"]) and xg["reference_frame_id"] == xw["reference_frame_id"] and xg["method"] == xw["method"]

        def matcher(b, d):
            tr = res[b]["tracking"]
            l0, l1 = int(plan_host[4, b]), int(plan_host[5, b])
            assert l0 == qs[b]["count"] and l1 == len(d["descriptors1"])
            if check_alone:      # the pair's matches0 equals the pair run alone
                one = _alone(net, data, b, l0, l1)
                assert torch.equal(tr["matches0"][:l0], one["matches0"][0]) and torch.equal(tr["matching_scores0"][:l0], one["matching_scores0"][0]), (t, b)
            return tr["matches0"][:l0].cpu().numpy()

        def solver(b, lists):
            tr = res[b]["tracking"]
            for k in TR.LIST_KEYS:      # the lists are bit-equal to the restatement fed with the device's matches0
                g, w = tr[k].cpu().numpy(), np.ascontiguousarray(lists[k])
                assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w.astype(g.dtype))), (t, b, k)
            assert tr["n_matches"] == len(lists["matched_keypoint_ids"])
            _check_pose(tr, lists, cams[b], b, f"[{tag}] step {t} stream {b} tracked")
            return {"success": tr["success"], "num_inliers": tr["num_inliers"], "inliers": tr["inliers"].cpu().numpy()}

        def refiner(b, frame, located, ret):
            x = res[b]["tracking"]["refinement"]
            assert x is not None and x["method"] == method
            if method == "matching":      # the stack over the covisible frames, from the tracker's inlier rows
                stack = RR.refine_stack(frame, scene["map"], dict(located, n_slots=RR.COVIS), lambda d, j: x["slots"][j]["matches0"].cpu().numpy(), scene["graph"])
                assert x["used_init"] == stack["used_init"]
                for k in RR.STACK_KEYS:
                    g = x[k].cpu().numpy()
                    assert np.array_equal(_bits(g), _bits(np.ascontiguousarray(stack[k]).astype(g.dtype))), (t, b, k)
            _check_pose(x, _np_lists(x), cams[b], b, f"[{tag}] step {t} stream {b} refined by {method}")
            return _np_refinement(x)

        def relocalizer(i, b, frame):
            assert rest[i] == b
            r = res[b]["localization"]
            if not r["success"]:
                return {"success": False}
            return dict(_np_lists(r), success=True, reference_frame_id=r["reference_frame_id"], refinement=_np_refinement(r["refinement"]))

        want = loop.step(qs, streams, matcher, solver, refiner, relocalizer, seg_ids=[q["seg_ids"] for q in qs])
        sources.append([r["source"] for r in res])
        assert sources[-1] == [w["source"] for w in want], (t, sources[-1])
        assert trk.lost.tolist() == loop.lost
        for b in streams:
            assert res[b]["success"] == want[b]["success"]
            if not res[b]["success"]:
                continue
            assert res[b]["reference_frame_id"] == want[b]["reference_frame_id"] == trk.reference_frame_id[b]
            if res[b]["source"] != "relocalize" and len(res[b]["matched_keypoint_ids"]) >= 64:
                p = scene["planted"][t][b]
                er, ec = PR.pose_errors(PR.qvec_to_rot(res[b]["qvec"]), res[b]["tvec"], p["R"], p["t"])
                print(f"track [{tag}]: step {t} stream {b} {res[b]['source']}: {er:.4f} deg, {ec:.4f} m from the planted camera, "
                      f"{res[b]['num_inliers']}/{len(res[b]['matched_keypoint_ids'])} inliers")
                assert er < 1.0 and ec < 0.5
        # the whole state
        exp = TR.state_arrays(loop, N_MAX, scene["index"])
        got = {k: getattr(trk.state, k).cpu().numpy() for k in STATE_KEYS}
        for s in streams:
            n = int(exp["counts"][s])
            assert got["counts"][s] == n and got["ref_frame"][s] == exp["ref_frame"][s] and np.array_equal(got["frame_norm"][s], exp["frame_norm"][s]), (t, s)
            for k in ("keypoints", "scores", "descriptors"):
                assert np.array_equal(_bits(got[k][s, :n]), _bits(exp[k][s, :n])), (t, s, k)
            for k in ("xyzs", "point3D_ids", "seg_ids"):
                assert np.array_equal(_bits(got[k][s]), _bits(exp[k][s])), (t, s, k)
        print(f"track [{tag}]: step {t}: sources {sources[-1]}, inliers {[r['num_inliers'] for r in res]}, lost {trk.lost.tolist()}")
    return sources, trk


def _assert_branches(sources):
    flat = [s for row in sources for s in row]
    assert "track" in flat and "track+refine" in flat
    assert any(sources[t][b] == "relocalize" and sources[t - 1][b] in ("track", "track+refine") for t in range(1, len(sources)) for b in range(TR.N_STREAMS))
    assert all(row[3] is None for row in sources)      # stream 3 (no keypoints) is lost in all three calls


@pytest.mark.parametrize("precision,method", [("x3", "matching"), ("f32", "projection")])
def test_public_call_gml(scene, dev, precision, method):
    """Three run calls on sequence_scene with GML: per query the pair's matches0 equals the pair run alone, the lists are bit-equal
    to the restatement fed with the device's matches0, the pose equals pose_ref.estimate_pose with the documented pair index
    inside 1e-8 / 2e-8, source / lost / reference_frame_id and the whole state equal the restatement's, a tracked query with 64
    matches or more stands within 1 degree / 0.5 m of its planted camera; relocalize equals localize_and_refine on the same
    sub-batch bit for bit; every branch is taken."""
    sources, _ = _run_sequence(scene, _gml(dev, precision), method, f"{precision} {method}")
    _assert_branches(sources)


@pytest.mark.parametrize("precision,method", [("x3", "projection"), ("f32", "matching")])
def test_public_call_gml_other_method(scene, dev, precision, method):
    """Both accurate precisions under both refinement methods."""
    sources, _ = _run_sequence(scene, _gml(dev, precision), method, f"{precision} {method}", check_alone=False)
    _assert_branches(sources)


def test_public_call_adagml(scene, dev):
    sources, _ = _run_sequence(scene, _adagml(dev), "matching", "adagml matching")
    assert all(row[3] is None for row in sources) and "relocalize" in sources[0]


def test_track_without_recognition_equals_runs_tracking_branch(scene, dev):
    """Two trackers brought to the same state by one run call; then run on one and track (no recognition) on the other: the
    tracking results are equal bit for bit, and so is the state on every row that carries a point."""
    net = _gml(dev)
    a, b = _tracker(scene, net), _tracker(scene, net)
    feats0, seg0 = scene["steps"][0]
    cams0 = [p["cam"] for p in scene["planted"][0]]
    a.run(feats0, seg0, cams0)
    b.run(feats0, seg0, cams0)
    feats1, seg1 = scene["steps"][1]
    cams1 = [p["cam"] for p in scene["planted"][1]]
    ra, rb = a.run(feats1, seg1, cams1), b.track(feats1, cams1)
    n_tracked = 0
    for s in range(TR.N_STREAMS):
        if rb[s] is None:
            assert ra[s]["tracking"] is None
            continue
        assert ra[s]["source"] == rb[s]["source"] and ra[s]["source"] in ("track", "track+refine")
        n_tracked += 1
        assert np.array_equal(ra[s]["qvec"], rb[s]["qvec"]) and np.array_equal(ra[s]["tvec"], rb[s]["tvec"]) and torch.equal(ra[s]["inliers"], rb[s]["inliers"])
        for k in TR.LIST_KEYS:
            assert torch.equal(ra[s][k], rb[s][k]), (s, k)
        has = a.state.point3D_ids[s] >= 0
        assert torch.equal(a.state.point3D_ids[s], b.state.point3D_ids[s]) and torch.equal(a.state.xyzs[s], b.state.xyzs[s])
        assert torch.equal(a.state.seg_ids[s][has], b.state.seg_ids[s][has]) and (b.state.seg_ids[s][~has] == -1).all()
    assert n_tracked == 3 and a.lost.tolist() == b.lost.tolist()
    b.reset([1])
    assert b.lost.tolist() == [False, True, False, True] and b.track(feats1, cams1)[1] is None


def test_ctypes_entries(hip_lib, dev):
    """The four entries through ctypes alone on hand-written tables, with every error status."""
    L = hip_lib
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    S, n_max, B, n = 3, 4, 2, 3
    s_kp = torch.arange(S * n_max * 2, dtype=torch.float32, device=dev).reshape(S, n_max, 2)
    s_sc, s_de = torch.zeros(S, n_max, device=dev), torch.zeros(S, n_max, 128, device=dev)
    s_xyz = torch.arange(S * n_max * 3, dtype=torch.float64, device=dev).reshape(S, n_max, 3) / 3
    s_p3d = i64([[5, -1, 7, 8], [0, 0, 0, 0], [-1, 21, 22, -1]])
    s_seg, s_cnt, s_ref, s_norm = i32(np.arange(S * n_max).reshape(S, n_max)), i32([4, 0, 3]), i32([9, 8, 7]), torch.ones(S, 3, device=dev)
    counts, slot = i32([3, 2]), i32([2, 0])
    plan, loc = i32(np.full((10, B), -9)), i32(np.full((10, B), -9))

    def run_plan(counts_=counts, plan_=plan, n_max_=n_max, batch=B):
        return L.pram_track_plan(p(counts_), p(slot), p(s_cnt), p(s_ref), batch, n, S, n_max_, p(plan_), p(loc), st)
    assert run_plan() == 0
    assert plan.cpu().tolist() == [[0, 1], [-1, -1], [2, 0], [0, 0], [3, 2], [3, 4], [-1, -1], [8, 0], [-1, -1], [0, 0]] and loc[2].tolist() == [7, 9]
    q_kp = torch.arange(B * n * 2, dtype=torch.float32, device=dev).reshape(B, n, 2) + 100
    m0 = i64([[1, 3, 0, 0], [2, 1, 0, 0]])      # query 0 (slot 2, 3 rows): 1 ok, 3 >= lens1, 0 has no point; query 1 (slot 0): 2 ok, 1 no point
    cap = 3
    o = {"ids": i64(np.full((B, cap), -5)), "kp": torch.zeros(B, cap, 2, device=dev), "rk": torch.zeros(B, cap, 2, device=dev), "p3": i64(np.full((B, cap), -5)),
         "xyz": torch.zeros(B, cap, 3, dtype=torch.float64, device=dev), "sid": i32(np.full((B, cap), -5))}
    m_count = i32([-5, -5])
    order = ("ids", "kp", "rk", "p3", "xyz", "sid")

    def run_cor(m0_=m0, ldm=4, t0=3, xyz_out=o["xyz"]):
        return L.pram_track_correspond(p(m0_), ldm, p(plan), p(q_kp), n, p(s_kp), p(s_xyz), p(s_p3d), p(s_seg), S, n_max, B, t0, cap, p(o["ids"]), p(o["kp"]),
                                       p(o["rk"]), p(o["p3"]), C.c_void_p(xyz_out.data_ptr()), p(o["sid"]), p(m_count), st)
    assert run_cor() == 0
    assert m_count.tolist() == [1, 1] and o["ids"][:, 0].tolist() == [0, 0] and o["p3"][:, 0].tolist() == [21, 7] and o["sid"][:, 0].tolist() == [9, 2]
    assert torch.equal(o["xyz"][0, 0], s_xyz[2, 1]) and torch.equal(o["rk"][1, 0], s_kp[0, 2]) and torch.equal(o["kp"][1, 0], q_kp[1, 0]) and o["ids"][0, 1:].tolist() == [-5, -5]
    # filter: keep row 0 of query 0, nothing of query 1
    f = {k: v.clone() for k, v in o.items()}
    f_count, mask = i32([-5, -5]), torch.tensor([[1, 1, 1], [0, 1, 1]], dtype=torch.uint8, device=dev)

    def run_filter(mask_=mask, first_out=f["ids"], cap_=cap):
        return L.pram_track_filter(*[p(o[k]) for k in order], p(m_count), p(mask_), B, cap_, p(first_out), *[p(f[k]) for k in order[1:]], p(f_count), st)
    assert run_filter() == 0
    assert f_count.tolist() == [1, 0] and f["p3"][0, 0].item() == 21
    # commit: query 0 -> slot 2, query 1 -> slot 0; list rows (0 -> keypoint 0), the repeated keypoint 1 of query 1: the last row wins
    q_sc, q_de = torch.ones(B, n, device=dev), torch.ones(B, n, 128, device=dev)
    c_ids, c_p3, c_sid, c_cnt = i64([[0, 9, 0], [1, 1, 5]]), i64([[31, 32, 33], [41, 42, 43]]), i32([[1, 2, 3], [4, 5, 6]]), i32([1, 3])
    c_xyz = torch.arange(B * 3 * 3, dtype=torch.float64, device=dev).reshape(B, 3, 3) + 50
    winner, ref_in = i32(np.full((B, n), 77)), i32([3, 4])
    host = (C.c_int * B)(2, 0)

    def run_commit(host_=host, q_de_=q_de, n_=n, winner_=winner):
        return L.pram_track_commit(p(q_kp), p(q_sc), p(q_de_), p(counts), None, p(slot), C.addressof(host_), p(ref_in), B, n_, 1.0, 2.0, 3.0, p(c_ids), p(c_p3),
                                   p(c_xyz), p(c_sid), p(c_cnt), None, 3, p(s_kp), p(s_sc), p(s_de), p(s_cnt), p(s_xyz), p(s_p3d), p(s_seg), p(s_ref), p(s_norm),
                                   S, n_max, p(winner_), st)
    assert run_commit() == 0
    assert s_cnt.tolist() == [2, 0, 3] and s_ref.tolist() == [4, 8, 3] and s_norm[2].tolist() == [1.0, 2.0, 3.0]
    assert s_p3d.tolist() == [[-1, 42, -1, -1], [0, 0, 0, 0], [31, -1, -1, -1]] and s_seg[0].tolist() == [-1, 5, -1, -1] and s_seg[2].tolist() == [1, -1, -1, -1]
    assert torch.equal(s_xyz[0, 1], c_xyz[1, 1]) and torch.equal(s_xyz[2, 0], c_xyz[0, 0]) and not s_xyz[0, 0].any() and torch.equal(s_kp[2, :3], q_kp[0])
    assert winner.tolist() == [[0, -1, -1], [-1, 1, -1]] and s_de[0, :2].eq(1).all() and s_de[0, 2:].eq(0).all()
    torch.cuda.synchronize()
    # error statuses: nothing is launched
    E_ARG = -1
    assert run_plan(counts_=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_plan(plan_=plan.view(torch.int8).view(-1)[1:]) == E_ARG and b"misaligned" in L.pram_last_error()
    assert run_plan(n_max_=-1) == E_ARG and run_plan(n_max_=2 ** 30) == E_ARG and b"32-bit" in L.pram_last_error()
    assert run_plan(batch=0) == 0
    assert run_cor(m0_=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_cor(m0_=m0.view(torch.int32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
    assert run_cor(xyz_out=o["xyz"].view(torch.float32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
    assert run_cor(ldm=2) == E_ARG and b"ldm" in L.pram_last_error()
    assert run_filter(mask_=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_filter(first_out=o["ids"]) == E_ARG and b"must not be the input" in L.pram_last_error()
    assert run_filter(cap_=-1) == E_ARG
    assert run_commit(host_=(C.c_int * B)(1, 1)) == E_ARG and b"name one slot" in L.pram_last_error()
    assert run_commit(host_=(C.c_int * B)(3, 0)) == E_ARG and b"outside" in L.pram_last_error()
    assert run_commit(q_de_=q_de.view(-1)[1:]) == E_ARG and b"16-byte" in L.pram_last_error()
    assert run_commit(n_=n_max + 1) == E_ARG and b"n <= n_max" in L.pram_last_error()
    assert run_commit(winner_=None) == E_ARG and b"null" in L.pram_last_error()
    assert s_cnt.tolist() == [2, 0, 3]


@pytest.mark.parametrize("mask_kind", ["seeded", "all", "none"])
def test_track_filter_chunk_and_wave_boundaries(dev, mask_kind):
    """List lengths at and around the wave's 64 and the workgroup's chunk of 256, and two chunks and one row (513); a seeded mask
    puts survivors on both sides of every boundary.  Bit-equal to numpy's boolean indexing, rows beyond the count untouched."""
    from pram_amd import ops
    rng = np.random.default_rng(29)
    counts = [63, 64, 65, 256, 257, 513]
    B, cap = len(counts), 513
    cor = {k: _random_bytes(rng, (B, cap) + tail, dt, dev) for k, dt, tail in zip(COR_KEYS, COR_DTYPES, COR_TAILS)}
    cor["count"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    mask = {"seeded": (rng.uniform(0, 1, (B, cap)) < 0.5).astype(np.uint8), "all": np.ones((B, cap), np.uint8), "none": np.zeros((B, cap), np.uint8)}[mask_kind]
    out = ops.track_filter(cor, torch.from_numpy(mask).to(dev), out=_sentinel_cor(B, cap, dev))
    sentinel = _sentinel_cor(B, cap, dev)
    for b in range(B):
        keep = np.nonzero(mask[b, :counts[b]])[0]
        assert int(out["count"][b]) == len(keep), (b, mask_kind)
        for k in COR_KEYS:
            assert np.array_equal(_bits(out[k][b, :len(keep)]), _bits(cor[k][b].cpu().numpy()[keep])), (b, k)
            assert np.array_equal(_bits(out[k][b, len(keep):]), _bits(sentinel[k][b, len(keep):])), (b, k)
