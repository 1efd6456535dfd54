"""GPU: pose refinement by matching over covisible frames (pram_amd.localization.refine, csrc/refine.hip) against the numpy
restatement tests/refine_ref.py: the three kernels on their own, the public call stage by stage, and the C entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import helpers as H
from tests import pose_ref as PR
from tests import refine_ref as RR

pytestmark = pytest.mark.gpu

E2E_Q_BAR, E2E_T_BAR = 1e-8, 2e-8      # the bars of tests/test_gpu_pose.py for the same kernels
LOC = dict(seg_k=RR.SEG_K, min_kpts=32, threshold=4.0, min_inliers=30, semantic_matching=False, trials=1000, seed=4)
COR_KEYS = ("matched_keypoint_ids", "matched_keypoints", "matched_ref_keypoints", "matched_point3D_ids", "matched_xyzs", "matched_sids")
COR_DTYPES = (torch.int64, torch.float32, torch.float32, torch.int64, torch.float64, torch.int32)
COR_TAILS = ((), (2,), (2,), (), (3,), ())


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


def _adagml(dev):
    from pram_amd.nets.adagml import AdaGML
    a = AdaGML({})
    a.load_state_dict(H.adagml_sd(), strict=True)
    return a.to(dev).eval()


def _real(q):
    return {k: (v[:q["count"]] if isinstance(v, np.ndarray) else v) for k, v in q.items() if k != "padded"}


@pytest.fixture(scope="module")
def scene(dev):
    from pram_amd.localization.candidates import ReferenceStore
    m, qs, planted = RR.covisible_scene()
    store = ReferenceStore(m["frames"], m["seg_ref_frame_ids"], m["start_sid"], device=dev, covisibility_frame=RR.COVIS)
    feats, seg = CR.batch_features(qs, dev)
    return {"map": m, "queries": qs, "planted": planted, "cams": [p["cam"] for p in planted], "store": store, "features": feats, "seg": seg,
            "graph": RR.covisibility_graph(m, RR.COVIS)}


def _localize(scene, net):
    from pram_amd.localization import pose
    kw = dict(LOC, overlap_ratio=0.5, min_inlier_ratio=0.01, refine_iters=20)
    return pose._localize(scene["features"], scene["seg"], scene["store"], net, scene["cams"], **kw)


def _expected_plan(sel, loc_host, counts, store, n_cov, enable):
    from pram_amd import ops
    f = ops.CAND_PLAN_FIELDS
    B = len(counts)
    seg_k = loc_host.shape[1] // B
    plan = np.zeros((ops.CAND_PLAN_COLS, B * n_cov), dtype=np.int32)
    ref, used, init = np.full(B, -1, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        kept, status = int(sel[b, 0]), int(sel[b, 1])
        fr = int(loc_host[f.index("frame"), b * seg_k + kept]) if kept >= 0 else -1
        sid = int(loc_host[f.index("sid"), b * seg_k + kept]) if kept >= 0 else -1
        live = fr >= 0 and (enable is None or bool(enable[b]))
        lst = store.covisible(fr)[:n_cov].tolist() if live else []
        for j in range(n_cov):
            g = lst[j] if j < len(lst) else -1
            rows = int(store.frame_off[g + 1] - store.frame_off[g]) if g >= 0 else 0
            plan[:, b * n_cov + j] = [b, sid, g, 0, counts[b] if g >= 0 else 0, rows, -1, int(store.frame_off[g]) if g >= 0 else 0, -1, j]
        ref[b], used[b], init[b] = (fr if live else -1), len(lst), int(live and status == 1 and fr in lst)
    return plan, ref, used, init


def test_store_tables_keep_their_old_keys(scene, dev):
    from pram_amd.localization.candidates import ReferenceStore
    m = scene["map"]
    t = ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0).tables(dev)
    old = {"descriptors", "keypoints", "scores", "xyzs", "point3D_ids", "keypoint_segs", "frame_norm", "sel_rows", "hist_label", "hist_cnt", "lm_frame",
           "lm_sel_off", "lm_sel_len", "frame_off", "hist_off", "n_rows", "n_frames", "n_landmarks", "start_sid"}
    new = {"pt_ids", "pt_off", "pt_frames", "is_vrf", "covis_off", "covis_frames", "covis_count", "n_points", "n_pt_entries", "n_covis", "covisibility_frame"}
    assert set(t) == old | new
    s = scene["store"]
    for name in ("pt_ids", "pt_off", "pt_frames", "is_vrf", "covis_off", "covis_frames", "covis_count"):
        host = getattr(s, name)
        got = s.tables(dev)[name].cpu().numpy()
        assert got.dtype == host.dtype and got.shape[0] == host.shape[0] + 1 and np.array_equal(got[:-1], host), name


def test_plan_exact(scene, dev):
    """Every column for every (query, slot) after a real localisation: lists cut to n_cov, empty slots beyond a short list, the
    query that was not located and the empty one, enable masking one query, init_on both ways."""
    from pram_amd import ops
    from pram_amd.localization.candidates import ReferenceStore
    out, state = _localize(scene, _gml(dev))
    sel, loc_host = state["sel"], state["plan"].cpu().numpy()
    counts = scene["features"]["counts"]
    cnt = counts.cpu().numpy()
    located = [b for b in range(len(cnt)) if sel[b, 0] >= 0]
    print("refine plan: chosen", sel.tolist())
    assert len(located) >= 3 and sel[4, 0] == -1 and cnt[4] == 0
    m = scene["map"]
    long_store = ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, device=dev, covisibility_frame=20)
    seen = set()
    for store, n_cov in ((scene["store"], RR.COVIS), (scene["store"], RR.COVIS + 2), (scene["store"], 2), (long_store, 8), (long_store, 1)):
        for enable in (None, [1, 0, 1, 1, 1], [0, 0, 0, 0, 0]):
            en = None if enable is None else torch.tensor(enable, dtype=torch.int32, device=dev)
            plan, ref, used, init = ops.refine_plan(state["chosen"], state["plan"], counts, store.tables(dev), n_cov, en)
            want = _expected_plan(sel, loc_host, cnt, store, n_cov, enable)
            for got, w, name in zip((plan, ref, used, init), want, ("plan", "ref_frame", "n_cov_used", "init_on")):
                assert np.array_equal(got.cpu().numpy(), w), (name, n_cov, enable, got.cpu().numpy().tolist(), w.tolist())
            p = dict(zip(ops.CAND_PLAN_FIELDS, want[0]))
            live = p["frame"] >= 0
            if ((want[2] > 0) & (want[2] < n_cov)).any():      # a list shorter than n_cov: the slots beyond it are empty
                seen.add("short_list")
            if enable is None:
                seen.update({"init_on"} if want[3].any() else set())
                seen.update({"init_off_located"} if any(want[3][b] == 0 for b in located) else set())
            assert (p["lens0"][~live] == 0).all() and (p["lens1"][~live] == 0).all() and (p["tok_off"] == -1).all() and (p["sel_off"] == -1).all()
            assert (want[1][4] == -1) and want[2][4] == 0
            if enable is not None and not enable[1]:
                assert want[1][1] == -1 and not live[n_cov:2 * n_cov].any()
    assert seen == {"short_list", "init_on", "init_off_located"}, seen


def _random_cor(rng, P, t, counts, dev):
    """pram_cand_correspond-shaped buffers with every bit random (xyz: random 64-bit words read as float64, NaN payloads among them)."""
    out = {}
    for k, dt, tail in zip(COR_KEYS, COR_DTYPES, COR_TAILS):
        nbytes = int(np.prod((P, t) + tail)) * torch.empty(0, dtype=dt).element_size()
        raw = torch.from_numpy(rng.integers(0, 256, nbytes, dtype=np.uint8))
        out[k] = raw.view(dt).reshape((P, t) + tail).to(dev)
    out["count"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    return out


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).reshape(-1).view(np.uint8)


def test_merge_exact(dev):
    """Crafted correspondences, no matcher: every field bit-equal to numpy concatenation in (slot ascending, then the
    localisation's rows); rows beyond the merged count keep the sentinel they were filled with."""
    from pram_amd import ops
    rng = np.random.default_rng(11)
    n_cov, seg_k, t0, t0a = 6, 2, 257, 64
    slot_counts = [[0, 1, 63, 0, 64, 65], [257, 0, 0, 257, 1, 0], [257] * 6, [0] * 6, [0, 0, 65, 0, 0, 1]]
    B = len(slot_counts)
    a_counts = [[5, 64], [64, 3], [17, 64], [9, 9], [0, 0]]
    chosen = [[1, 1, 1], [0, 0, 0], [1, 1, 1], [-1, -1, -1], [0, 1, 0]]
    init_on = [1, 0, 1, 0, 1]                                   # query 2 fills cap exactly; query 4: init on, nothing to append
    cap = n_cov * t0 + t0a
    r = _random_cor(rng, B * n_cov, t0, [c for row in slot_counts for c in row], dev)
    a = _random_cor(rng, B * seg_k, t0a, [c for row in a_counts for c in row], dev)
    ch = torch.tensor(chosen, dtype=torch.int32, device=dev)
    io = torch.tensor(init_on, dtype=torch.int32, device=dev)
    fill = lambda: {**{k: torch.from_numpy(np.full(int(np.prod((B, cap) + tail)) * torch.empty(0, dtype=dt).element_size(), 0xA5, np.uint8)).view(dt)
                       .reshape((B, cap) + tail).to(dev) for k, dt, tail in zip(COR_KEYS, COR_DTYPES, COR_TAILS)},
                    "matched_src": torch.full((B, cap), -7, dtype=torch.int32, device=dev), "count": torch.full((B,), -7, dtype=torch.int32, device=dev)}
    out = ops.refine_merge(r, a, ch, io, n_cov, out=fill())
    sentinel = fill()
    counts = out["count"].cpu().numpy()
    for b in range(B):
        segs = [(r, b * n_cov + j, slot_counts[b][j], j) for j in range(n_cov)]
        if init_on[b]:
            segs.append((a, b * seg_k + chosen[b][0], a_counts[b][chosen[b][0]], n_cov))
        total = sum(s[2] for s in segs)
        assert counts[b] == total, (b, counts[b], total)
        for k in COR_KEYS:
            want = torch.cat([src[k][p, :c] for src, p, c, _ in segs])
            assert np.array_equal(_bits(out[k][b, :total]), _bits(want)), (b, k)
            assert np.array_equal(_bits(out[k][b, total:]), _bits(sentinel[k][b, total:])), (b, k, "rows beyond the count were written")
        assert out["matched_src"][b, :total].cpu().tolist() == [j for _, _, c, j in segs for _ in range(c)]
        assert (out["matched_src"][b, total:] == -7).all()
    assert counts[2] == cap and counts[3] == 0 and counts[4] == 66
    # the default path allocates [B, cap] itself and agrees
    again = ops.refine_merge(r, a, ch, io, n_cov)
    assert again["matched_xyzs"].shape == (B, cap, 3) and torch.equal(again["count"], out["count"])
    for b in range(B):
        assert np.array_equal(_bits(again["matched_xyzs"][b, :counts[b]]), _bits(out["matched_xyzs"][b, :counts[b]]))


def _vote_map(seed=5, n_frames=12, n_points=300):
    rng = np.random.default_rng(seed)
    fr = lambda fid, ids: {"id": fid, "keypoints": np.zeros((len(ids), 3), np.float32), "descriptors": np.zeros((len(ids), 128), np.float32),
                           "xyzs": np.zeros((len(ids), 3)), "point3D_ids": np.array(ids, dtype=np.int64),
                           "keypoint_segs": np.zeros(len(ids), np.int32), "width": 640, "height": 480}
    ids = (rng.permutation(5000)[:n_points] * 7 + 3).astype(np.int64)
    # lists of 1 .. 6 frames, duplicates among them; frames 3 and 8 are nobody's reference frame
    p2f = {int(i): (50 + rng.integers(0, n_frames, rng.integers(1, 7))).tolist() for i in ids}
    frames = [fr(50 + f, ids[f * 5:f * 5 + 5].tolist()) for f in range(n_frames)]
    vrf = [f for f in range(n_frames) if f not in (3, 8)]
    return {"frames": frames, "seg_ref_frame_ids": {l: [50 + f, 50 + vrf[(l + 1) % len(vrf)]] for l, f in enumerate(vrf)}, "start_sid": 0,
            "point3D_frame_ids": p2f}, ids


def test_frame_vote_exact(dev):
    """find_reference_frames per query against the restatement: multiplicity of ids and of lists, frames that are nobody's
    reference frame ignored, ids the map does not know, ties in the canonical order, success = 0 taking all rows, k below and
    above the number of voted frames, a query without rows; twice, bit-equal."""
    from pram_amd import ops
    from pram_amd.localization.candidates import ReferenceStore
    m, ids = _vote_map()
    store = ReferenceStore(m["frames"], m["seg_ref_frame_ids"], 0, device=dev, point3D_frame_ids=m["point3D_frame_ids"], covisibility_frame=4)
    vrf = RR.vrf_frame_ids(m)
    assert len(vrf) == 10 and 53 not in vrf and 58 not in vrf
    rng = np.random.default_rng(6)
    cap = 700
    counts = [700, 300, 0, 40, 3, 1, 257]
    success = [1, 0, 1, 1, 0, 1, 1]
    B = len(counts)
    pool = np.concatenate([ids, np.array([-1, 1, 2, 10 ** 12, ids.max() + 1])])      # the last five: ids the map does not know
    mp = rng.choice(pool, (B, cap))
    mp[3, :40] = rng.choice(ids[:6], 40)                                             # few points, many times: high multiplicity, ties
    mp[5, 0] = 2                                                                     # one row, unknown id: an empty vote
    inl = (rng.uniform(0, 1, (B, cap)) < 0.6).astype(np.uint8)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    args = (t(mp, torch.int64), t(np.array(counts), torch.int32), t(inl, torch.uint8), t(np.array(success), torch.int32), store.tables(dev))
    ties = 0
    for k in (1, 3, 12):
        bf, bc, nb = (x.cpu().numpy() for x in ops.refine_frame_vote(*args, k))
        bf2, bc2, nb2 = (x.cpu().numpy() for x in ops.refine_frame_vote(*args, k))
        assert np.array_equal(bf, bf2) and np.array_equal(bc, bc2) and np.array_equal(nb, nb2)
        for b in range(B):
            rows = mp[b, :counts[b]]
            want = RR.find_reference_frames(m, rows[inl[b, :counts[b]] != 0] if success[b] else rows, vrf, with_counts=True)
            ties += len({c for _, c in want}) < len(want)
            n = min(k, len(want))
            assert nb[b] == n, (k, b, nb[b], n)
            assert [store.frame_ids[i] for i in bf[b, :n]] == [g for g, _ in want[:n]] and bc[b, :n].tolist() == [c for _, c in want[:n]], (k, b)
            assert (bf[b, n:] == -1).all() and (bc[b, n:] == 0).all()
        assert nb[2] == 0 and nb[5] == 0 and (k < 10) == bool(nb[0] == k) and nb[0] <= 10
    assert ties > 0


def _alone(net, data, p, l0, l1):
    one = {}
    for side, l in (("0", l0), ("1", l1)):
        for key in ("descriptors", "norm_keypoints", "scores"):
            one[key + side] = data[key + side][p:p + 1, :l].contiguous()
        one["keypoints" + side] = one["norm_keypoints" + side]
    return net.produce_matches(one)


def _refine_data(scene, net, n_cov):
    """the grouped call's inputs, rebuilt outside the public call: for the pairs run alone"""
    from pram_amd import ops
    from pram_amd.localization import candidates as cd
    _, state = _localize(scene, net)
    plan = ops.refine_plan(state["chosen"], state["plan"], scene["features"]["counts"], scene["store"].tables(state["chosen"].device), n_cov)[0]
    return cd.gather_candidates(scene["features"], {"plan": plan, "vote": {"tokens": state["tokens"]}}, scene["store"])


def _check_slots_alone(scene, net, res, n_cov):
    data = _refine_data(scene, net, n_cov)
    pairs = matches = 0
    for b, r in enumerate(res):
        x = r["refinement"]
        if x is None:
            continue
        for j, s in enumerate(x["slots"]):
            one = _alone(net, data, b * n_cov + j, s["n_query_kpts"], s["n_ref_kpts"])
            assert torch.equal(s["matches0"], one["matches0"][0]) and torch.equal(s["matching_scores0"], one["matching_scores0"][0]), (b, j)
            assert int(s["n_matches"]) == int((s["matches0"] >= 0).sum())
            pairs += 1
            matches += int(s["n_matches"])
    return pairs, matches


def _same_localisation(a, b):
    for ra, rb in zip(a, b):
        for k in ("success", "tracking_status", "num_inliers", "order", "reference_frame_id", "sid"):
            assert ra[k] == rb[k], k
        if ra["success"]:
            assert np.array_equal(ra["qvec"], rb["qvec"]) and np.array_equal(ra["tvec"], rb["tvec"]) and torch.equal(ra["inliers"], rb["inliers"])
            for k in ra:
                if k.startswith("matched_"):
                    assert torch.equal(ra[k], rb[k]), k
        for ca, cb in zip(ra["candidates"], rb["candidates"]):
            assert ca["success"] == cb["success"] and ca["num_inliers"] == cb["num_inliers"] and np.array_equal(ca["qvec"], cb["qvec"])
            assert np.array_equal(ca["tvec"], cb["tvec"]) and torch.equal(ca["matches0"], cb["matches0"]) and torch.equal(ca["matching_scores0"], cb["matching_scores0"])


def _same_refinement(x, y):
    assert (x is None) == (y is None)
    if x is None:
        return
    for k, v in x.items():
        if k == "slots":
            for sx, sy in zip(v, y[k]):
                assert torch.equal(sx["matches0"], sy["matches0"]) and torch.equal(sx["matching_scores0"], sy["matching_scores0"])
        elif torch.is_tensor(v):
            assert torch.equal(v, y[k]), k
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, y[k]), k
        else:
            assert v == y[k], k


@pytest.mark.parametrize("precision", ["x3", "f32"])
def test_public_call(scene, dev, precision):
    """localize_and_refine on covisible_scene: every (query, covisible frame) pair's matches0 equals the pair run alone; the merged
    lists equal the restatement's stack built from those matches0; the pose equals pose_ref.estimate_pose on the device's own
    merged list with p = b; the frame vote equals the restatement's; a refined tracked query stands at its planted camera;
    localize_candidates before and after is bit-equal.

    Inliers / matches of the localisation -> of the refinement (MI355X, seed 7, both precisions; printed, not asserted beyond the
    equality with the restatement): query 0 105 / 110 -> 354 / 378, query 1 55 / 68 -> 200 / 275, query 2 49 / 58 -> 162 / 240,
    query 3 (not tracked) 4 / 7 -> 7 / 23; DESIGN.md 4.13."""
    from pram_amd.localization.pose import localize_candidates
    from pram_amd.localization.refine import localize_and_refine
    net = _gml(dev, precision)
    s, n_cov = scene, RR.COVIS
    args = (s["features"], s["seg"], s["store"], net, s["cams"])
    before = localize_candidates(*args, **LOC)
    res = localize_and_refine(*args, **LOC)
    after = localize_candidates(*args, **LOC)
    _same_localisation(before, after)
    _same_localisation(before, res)
    pairs, matches = _check_slots_alone(s, net, res, n_cov)
    ids = RR.frame_ids(s["map"])
    n_refined = n_tracked = 0
    for b, r in enumerate(res):
        x = r["refinement"]
        assert (x is None) == (not r["success"]), b
        if x is None:
            continue
        n_refined += 1
        q = _real(s["queries"][b])
        located = {k: v.cpu().numpy() for k, v in r.items() if k.startswith("matched_")}
        located.update(reference_frame_id=r["reference_frame_id"], tracking_status=r["tracking_status"], n_slots=n_cov)
        slots = x["slots"]
        stack = RR.refine_stack(q, s["map"], located, lambda d, j: slots[j]["matches0"].cpu().numpy(), s["graph"])
        assert [sl["reference_frame_id"] for sl in slots] == stack["db_ids"] and x["n_covisible"] == len(stack["db_ids"])
        assert x["used_init"] == stack["used_init"]
        n = len(stack["matched_keypoint_ids"])
        assert n < 1000
        for k in RR.STACK_KEYS + ("matched_src",):
            g = x[k].cpu().numpy()
            w = np.ascontiguousarray(stack[k]).astype(g.dtype)
            assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (b, k, g.shape, w.shape)
        ref = PR.estimate_pose(x["matched_keypoints"].cpu().numpy(), x["matched_xyzs"].cpu().numpy(), s["cams"][b], threshold=LOC["threshold"],
                               trials=LOC["trials"], refine_iters=20, seed=LOC["seed"], p=b)
        assert x["success"] == ref["success"] and x["num_inliers"] == ref["num_inliers"], (b, x["num_inliers"], ref["num_inliers"])
        assert np.array_equal(x["inliers"].cpu().numpy(), ref["inliers"]), b
        dq = float(np.abs(x["qvec"] - ref["qvec"]).max())
        dt = float(np.abs(x["tvec"] - ref["tvec"]).max() / (1.0 + np.abs(ref["tvec"]).max()))
        print(f"refine [{precision}]: query {b} ref frame {r['reference_frame_id']} status {r['tracking_status']} init {x['used_init']}: inliers "
              f"{r['num_inliers']}/{r['matched_keypoints'].shape[0]} -> {x['num_inliers']}/{n} over {x['n_covisible']} frames, success "
              f"{x['success']}, dq {dq:.2e} dt {dt:.2e}, new frames {x['refinement_reference_frame_ids']}")
        assert dq <= E2E_Q_BAR and dt <= E2E_T_BAR, (b, dq, dt)
        p3d = stack["matched_point3D_ids"]
        best = RR.find_reference_frames(s["map"], p3d[ref["inliers"]] if ref["success"] else p3d, s["graph"].keys())
        assert x["refinement_reference_frame_ids"] == best[:n_cov], (b, x["refinement_reference_frame_ids"], best)
        assert x["reference_frame_id"] == (best[0] if best else r["reference_frame_id"]) and all(fid in ids for fid in best)
        if r["tracking_status"] and x["success"]:
            n_tracked += 1
            er, ec = PR.pose_errors(PR.qvec_to_rot(x["qvec"]), x["tvec"], s["planted"][b]["R"], s["planted"][b]["t"])
            e0 = PR.pose_errors(PR.qvec_to_rot(r["qvec"]), r["tvec"], s["planted"][b]["R"], s["planted"][b]["t"])
            print(f"refine [{precision}]: query {b} refined: {er:.4f} deg, {ec:.4f} m from the planted camera (localisation: {e0[0]:.4f} deg, {e0[1]:.4f} m)")
            assert er < 1.0 and ec < 0.5
    print(f"refine [{precision}]: {n_refined} refined queries, {n_tracked} tracked, {pairs} pairs, {matches} matches")
    assert n_refined >= 3 and n_tracked >= 2 and pairs == n_refined * n_cov and res[4]["refinement"] is None
    # enable: the masked query is not refined, the others are what they were
    masked = localize_and_refine(*args, **LOC, enable=[True, False, True, True, True])
    assert masked[1]["refinement"] is None
    for b in (0, 2, 3, 4):
        _same_refinement(res[b]["refinement"], masked[b]["refinement"])


def test_adagml_grouped_equals_alone(scene, dev):
    from pram_amd.localization.refine import localize_and_refine
    net = _adagml(dev)
    res = localize_and_refine(scene["features"], scene["seg"], scene["store"], net, scene["cams"], **LOC)
    pairs, matches = _check_slots_alone(scene, net, res, RR.COVIS)
    print(f"refine [adagml]: {pairs} pairs, {matches} matches")
    assert pairs >= RR.COVIS


def test_determinism(scene, dev):
    from pram_amd.localization.refine import localize_and_refine
    net = _gml(dev)
    args = (scene["features"], scene["seg"], scene["store"], net, scene["cams"])
    a, b = localize_and_refine(*args, **LOC), localize_and_refine(*args, **LOC)
    _same_localisation(a, b)
    assert any(r["refinement"] is not None for r in a)
    for ra, rb in zip(a, b):
        _same_refinement(ra["refinement"], rb["refinement"])


def test_ctypes_entries(hip_lib, dev):
    """The three entries through ctypes alone on hand-written tables, with every error status."""
    L = hip_lib
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # three frames of 4, 2, 3 rows; covisible lists: frame 0 -> [0, 2], frame 1 -> [], frame 2 -> [2, 0, 1]
    frame_off, covis_off, covis_frames = i32([0, 4, 6, 9]), i32([0, 2, 2, 5]), i32([0, 2, 2, 0, 1])
    # two queries, seg_k = 2: query 0 kept candidate 1 (frame 2, sid 7, tracked), query 1 kept candidate 0 (frame 0, sid 3, not tracked)
    chosen, counts = i32([[1, 1, 1], [0, 0, 0]]), i32([5, 6])
    loc_plan = torch.zeros(10, 4, dtype=torch.int32, device=dev)
    loc_plan[1], loc_plan[2] = i32([9, 7, 3, 4]), i32([1, 2, 0, 1])
    n_cov = 3
    plan = torch.full((10, 2 * n_cov), -9, dtype=torch.int32, device=dev)
    ref, used, init = i32([-9, -9]), i32([-9, -9]), i32([-9, -9])

    def run_plan(n_cov=n_cov, chosen_=chosen, enable=None, n_frames=3):
        return L.pram_refine_plan(p(chosen_) if chosen_ is not None else None, p(loc_plan), p(counts), p(enable) if enable is not None else None,
                                  p(frame_off), p(covis_off), p(covis_frames), 2, 2, n_cov, n_frames, 5, p(plan), p(ref), p(used), p(init), st)
    assert run_plan() == 0
    want = [[0, 0, 0, 1, 1, 1], [7, 7, 7, 3, 3, 3], [2, 0, 1, 0, 2, -1], [0] * 6, [5, 5, 5, 6, 6, 0], [3, 4, 2, 4, 3, 0], [-1] * 6, [6, 0, 4, 0, 6, 0],
            [-1] * 6, [0, 1, 2, 0, 1, 2]]
    assert plan.cpu().tolist() == want and ref.tolist() == [2, 0] and used.tolist() == [3, 2] and init.tolist() == [1, 0]
    assert run_plan(enable=i32([0, 1])) == 0
    assert ref.tolist() == [-1, 0] and used.tolist() == [0, 2] and init.tolist() == [0, 0] and plan[2].tolist() == [-1, -1, -1, 0, 2, -1]
    # merge: t0 = 2, t0a = 2, cap = 8
    t0, t0a, cap = 2, 2, 8
    mk = lambda P, t, base: {"ids": i64(np.arange(P * t).reshape(P, t) + base), "kp": torch.arange(P * t * 2, dtype=torch.float32, device=dev).reshape(P, t, 2) + base,
                             "rk": torch.arange(P * t * 2, dtype=torch.float32, device=dev).reshape(P, t, 2) - base, "p3": i64(np.arange(P * t).reshape(P, t) * 10 + base),
                             "xyz": torch.arange(P * t * 3, dtype=torch.float64, device=dev).reshape(P, t, 3) / 7 + base, "sid": i32(np.arange(P * t).reshape(P, t) % 5)}
    r, a = mk(2 * n_cov, t0, 100), mk(4, t0a, 500)
    r_count, a_count, init_on = i32([2, 0, 1, 0, 0, 2]), i32([1, 2, 2, 1]), i32([1, 0])
    o = {"ids": i64(np.full((2, cap), -5)), "kp": torch.zeros(2, cap, 2, device=dev), "rk": torch.zeros(2, cap, 2, device=dev), "p3": i64(np.full((2, cap), -5)),
         "xyz": torch.zeros(2, cap, 3, dtype=torch.float64, device=dev), "sid": i32(np.full((2, cap), -5)), "src": i32(np.full((2, cap), -5))}
    m_count = i32([-5, -5])
    order = ("ids", "kp", "rk", "p3", "xyz", "sid")

    def run_merge(n_cov=n_cov, cap=cap, first=r["ids"], xyz_out=o["xyz"]):
        return L.pram_refine_merge(p(first) if first is not None else None, *[p(r[k]) for k in order[1:]], p(r_count), t0, *[p(a[k]) for k in order], p(a_count), t0a,
                                   p(chosen), p(init_on), 2, 2, n_cov, cap, *[p(o[k]) for k in order[:4]], C.c_void_p(xyz_out.data_ptr()), p(o["sid"]),
                                   p(o["src"]), p(m_count), st)
    assert run_merge() == 0
    assert m_count.tolist() == [5, 2]
    assert o["ids"][0, :5].tolist() == [100, 101, 104, 502, 503] and o["src"][0, :5].tolist() == [0, 0, 2, 3, 3] and o["ids"][0, 5:].tolist() == [-5] * 3
    assert o["ids"][1, :2].tolist() == [110, 111] and o["src"][1, :2].tolist() == [2, 2] and o["src"][1, 2:].tolist() == [-5] * 6
    assert torch.equal(o["xyz"][0, :5], torch.cat([r["xyz"][0], r["xyz"][2, :1], a["xyz"][1]])) and torch.equal(o["kp"][0, 3:5], a["kp"][1])
    assert torch.equal(o["p3"][0, :5], torch.cat([r["p3"][0], r["p3"][2, :1], a["p3"][1]])) and torch.equal(o["sid"][1, :2], r["sid"][5])
    # vote: points 11 -> frames [0, 2, 2], 12 -> [1], 15 -> [2, 0]; frame 1 is nobody's reference frame
    pt_ids, pt_off, pt_frames, is_vrf = i64([11, 12, 15]), i32([0, 3, 4, 6]), i32([0, 2, 2, 1, 2, 0]), i32([1, 0, 1])
    m_p3d = i64([[11, 15, 12, 99, 11, 0, 0, 0], [15, 12, 0, 0, 0, 0, 0, 0]])
    inl = torch.tensor([[1, 1, 1, 1, 0, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.uint8, device=dev)
    succ = i32([1, 0])
    hist = i32(np.full((2, 3), 77))
    bf, bc, nb = i32(np.full((2, 2), -9)), i32(np.full((2, 2), -9)), i32([-9, -9])

    def run_vote(k=2, n_frames=3, ids=m_p3d, hist_=hist):
        return L.pram_refine_frame_vote(C.c_void_p(ids.data_ptr()), p(m_count), p(inl), p(succ), 2, 8, p(pt_ids), p(pt_off), p(pt_frames), 3, 6, p(is_vrf),
                                        n_frames, k, p(hist_) if hist_ is not None else None, p(bf), p(bc), p(nb), st)
    assert run_vote() == 0      # query 0: rows 0 .. 4, inliers only: 11, 15 (12 votes for frame 1 only, 99 unknown, the second 11 is no inlier)
    assert hist.tolist() == [[2, 0, 3], [1, 0, 1]] and bf.tolist() == [[2, 0], [0, 2]] and bc.tolist() == [[3, 2], [1, 1]] and nb.tolist() == [2, 2]
    torch.cuda.synchronize()
    # error statuses: nothing is launched
    E_ARG = -1
    assert run_plan(n_cov=0) == E_ARG and b"n_cov" in L.pram_last_error()
    assert run_plan(n_cov=-3) == E_ARG
    assert run_plan(chosen_=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_plan(n_frames=-1) == E_ARG
    assert run_merge(n_cov=0) == E_ARG and b"n_cov" in L.pram_last_error()
    assert run_merge(cap=7) == E_ARG and b"cap" in L.pram_last_error()
    assert run_merge(first=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_merge(xyz_out=o["xyz"].view(torch.float32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
    assert run_vote(k=4) == E_ARG and b"k <= n_frames" in L.pram_last_error()
    assert run_vote(k=0) == E_ARG
    assert run_vote(hist_=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_vote(ids=m_p3d.view(torch.int32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
