"""GPU: pose refinement by projection over covisible frames (pram_amd.localization.refine.refine_by_projection,
csrc/projref.hip) against the numpy restatement tests/projref_ref.py, whose matching is the reference's DENSE formula: the four
kernels on their own, the public call stage by stage, the method switch of localize_and_refine, and the C entries.  No decision
is excused: tests/test_refine_projection_cpu.py asserts that every decision of these inputs stands clear of its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import pose_ref as PR
from tests import projref_ref as PJ
from tests import refine_ref as RR
from tests import test_gpu_refine as TGR

pytestmark = pytest.mark.gpu

E2E_Q_BAR, E2E_T_BAR = 1e-8, 2e-8      # DESIGN.md 4.12's bars for the pose kernels
D_BAR = 1e-4                            # the bar tests/test_edges.py::test_hip_projection_refinement puts on the distances
MATCH_SEED = 10
POSE = dict(trials=1000, refine_iters=20, seed=4)


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)


def _store(map_, dev, **kw):
    from pram_amd.localization.candidates import ReferenceStore
    return ReferenceStore(map_["frames"], map_["seg_ref_frame_ids"], map_.get("start_sid", 0), device=dev, point3D_frame_ids=map_.get("point3D_frame_ids"), **kw)


def _state(entries, store, dev, seg_k=2):
    """What pose._localize leaves on the device, written by hand: entries[i] = dict(reference_frame_id or None, kept, qvec, tvec).
    The slot that was not kept carries another frame and a NaN pose: reading it shows."""
    from pram_amd import ops
    B = len(entries)
    index = {fid: i for i, fid in enumerate(store.frame_ids)}
    chosen = np.full((B, 3), -1, np.int32)
    plan = np.zeros((ops.CAND_PLAN_COLS, B * seg_k), np.int32)
    plan[ops.CAND_PLAN_FIELDS.index("frame")] = (np.arange(B * seg_k) * 3 + 1) % max(store.n_frames, 1)
    qvec, tvec = np.full((B * seg_k, 4), np.nan), np.full((B * seg_k, 3), np.nan)
    for b, e in enumerate(entries):
        if e is None or e["reference_frame_id"] is None:
            continue
        kept = e.get("kept", b % seg_k)
        chosen[b] = [kept, 1, kept]
        plan[ops.CAND_PLAN_FIELDS.index("frame"), b * seg_k + kept] = index[e["reference_frame_id"]]
        qvec[b * seg_k + kept], tvec[b * seg_k + kept] = e["qvec"], e["tvec"]
    return {"chosen": _t(chosen, torch.int32, dev), "plan": _t(plan, torch.int32, dev), "seg_k": seg_k,
            "est": {"qvec": _t(qvec, torch.float64, dev), "tvec": _t(tvec, torch.float64, dev)}}


def _cams(cams, dev):
    from pram_amd.localization import pose
    from pram_amd.localization.refine import image_size_table
    return pose.device_cameras(cams, dev), _t(image_size_table(cams), torch.int32, dev)


@pytest.mark.parametrize("n_points", [1, 31, 32, 33, 1000])
def test_mark_project_exact(dev, n_points):
    """pram_projref_mark + pram_projref_project against the restatement on mark_map: rows with id -1 and with ids outside the
    point table, a reference frame outside its own list (frame 50) and inside, the lists whole (n_cov 4) and cut (n_cov 2), a
    query that is not located and one that is disabled, every camera model, a query that sees nothing (n_cand 0); with 1000
    points: points behind the camera, beyond 100 m and outside each image edge.  cand_pt, n_union, n_cand exact, cand_uv 1e-9;
    twice, bit-equal."""
    from pram_amd import ops
    map_, queries = PJ.mark_map(n_points, 40 + n_points)
    store = _store(map_, dev, covisibility_frame=4)
    tables = store.point_tables(dev)
    assert int(tables["n_points"]) == n_points and tuple(tables["pt_xyz"].shape) == (n_points + 1, 3) and tuple(tables["pt_desc"].shape) == (n_points + 1, 128)
    state = _state(queries, store, dev)
    (cam_model, cam_params, _), sizes = _cams([q["cam"] for q in queries], dev)
    enable = _t(np.array([q["enable"] for q in queries]), torch.int32, dev)
    seen = set()
    for n_cov in (4, 2):
        want = PJ.mark_expected(map_, queries, n_cov)
        cap = max(1, min(n_points, (n_cov + 1) * store.max_frame_rows))
        runs = []
        for _ in range(2):
            bitmap, ref_frame = ops.projref_mark(state["chosen"], state["plan"], tables, n_cov, enable)
            cand_pt, cand_uv, n_union, n_cand = ops.projref_project(bitmap, state["chosen"], state["est"]["qvec"], state["est"]["tvec"], cam_model, cam_params,
                                                                    sizes, tables, cap)
            runs.append([x.cpu().numpy() for x in (bitmap, ref_frame, cand_pt, cand_uv, n_union, n_cand)])
        bitmap, ref_frame, cand_pt, cand_uv, n_union, n_cand = runs[0]
        for b, w in enumerate(want):
            if w is None:
                assert ref_frame[b] == -1 and n_union[b] == 0 and n_cand[b] == 0 and not bitmap[b].any(), (n_cov, b)
                continue
            n = len(w["cand"])
            assert store.frame_ids[ref_frame[b]] == queries[b]["reference_frame_id"]
            bits = np.zeros(bitmap.shape[1] * 32, bool)
            bits[w["union"]] = True
            assert np.array_equal(np.unpackbits(bitmap[b].view(np.uint8), bitorder="little").astype(bool), bits), (n_cov, b)
            assert n_union[b] == len(w["union"]) and n_cand[b] == n, (n_cov, b, n_union[b], len(w["union"]), n_cand[b], n)
            assert np.array_equal(cand_pt[b, :n], w["cand"]), (n_cov, b)
            assert n == 0 or np.abs(cand_uv[b, :, :n] - w["uv"]).max() <= 1e-9, (n_cov, b)
            assert np.array_equal(runs[1][2][b, :n], cand_pt[b, :n]) and np.array_equal(runs[1][3][b, :, :n], cand_uv[b, :, :n])
            seen.add("listed" if w["listed"] else "unlisted")
            seen.update({"cut"} if (n_cov == 2 and w["list_len"] == 2) else set())
            seen.update({"n_cand_0"} if (n == 0 and len(w["union"])) else set())
            cam = queries[b]["cam"]
            for name, hit in (("behind", w["depth"] <= 0), ("beyond", w["depth"] >= 100), ("left", (w["depth"] > 0) & (w["u"] < 0)),
                              ("right", (w["depth"] > 0) & (w["u"] >= cam[1])), ("above", (w["depth"] > 0) & (w["v"] < 0)),
                              ("below", (w["depth"] > 0) & (w["v"] >= cam[2]))):
                seen.update({name} if hit.any() else set())
        for a, c in zip(runs[0][:2] + runs[0][4:], runs[1][:2] + runs[1][4:]):
            assert np.array_equal(a, c)
    print(f"mark / project, {n_points} points: {sorted(seen)}")
    if n_points == 1000:
        assert seen == {"listed", "unlisted", "cut", "n_cand_0", "behind", "beyond", "left", "right", "above", "below"}, seen
    assert want[2] is None and want[3] is None      # not located; disabled


def test_project_two_sweeps_and_three_chunks(dev):
    """pram_projref_project alone on hand-made bitmaps over 32 * 1024 + 33 points: the bitmap is two sweeps of 1024 words long and
    its last word holds one point (the bits beyond it are set and must not count).  Query 0 marks 300 points, among them the
    first and last of a word, of a wave's 64 words and of each sweep; query 1 marks 2500, so the projection compacts in place over
    three chunks of 1024 candidates; query 2 is not located.  n_union, n_cand and cand_pt exact against projref_ref.project, cand_uv
    1e-9 (test_mark_project_exact's bar)."""
    from pram_amd import ops
    rng = np.random.default_rng(61)
    n_points = 32 * 1024 + 33
    words = (n_points + 31) // 32
    edge = np.array([0, 31, 32, 2047, 2048, 32767, 32768, 32799, 32800])
    pool = np.setdiff1d(np.arange(n_points), edge)
    marks = [np.sort(np.concatenate([edge, rng.choice(pool, k - len(edge), replace=False)])) for k in (300, 2500)]
    bits = np.zeros((3, words * 32), bool)
    bits[0, marks[0]], bits[1, marks[1]] = True, True
    bits[:, n_points:] = True
    bitmap = _t(np.packbits(bits, axis=1, bitorder="little").view(np.int32), torch.int32, dev)
    xyz = np.stack([rng.uniform(-40, 40, n_points), rng.uniform(-30, 30, n_points), rng.uniform(-30, 160, n_points)], 1)
    tables = {"pt_xyz": _t(xyz, torch.float64, dev), "n_points": n_points}
    cams = [PJ.MARK_CAMERAS[0], PJ.MARK_CAMERAS[1], PJ.MARK_CAMERAS[4]]
    (cam_model, cam_params, _), sizes = _cams(cams, dev)
    B, seg_k, cap = 3, 2, 2500
    chosen = np.array([[0, 1, 0], [1, 1, 1], [-1, 0, -1]], np.int32)
    qvec, tvec = np.full((B * seg_k, 4), np.nan), np.full((B * seg_k, 3), np.nan)
    for b in range(2):
        qvec[b * seg_k + chosen[b, 0]] = PR.rot_to_qvec(PR.rodrigues(rng.standard_normal(3) * 0.05))
        tvec[b * seg_k + chosen[b, 0]] = rng.standard_normal(3) * 0.5
    cand_pt, cand_uv, n_union, n_cand = (x.cpu().numpy() for x in ops.projref_project(
        bitmap, _t(chosen, torch.int32, dev), _t(qvec, torch.float64, dev), _t(tvec, torch.float64, dev), cam_model, cam_params, sizes, tables, cap))
    assert n_union[2] == 0 and n_cand[2] == 0
    for b in range(2):
        row, cam = b * seg_k + chosen[b, 0], cams[b]
        u, v, _, mask = PJ.project(xyz[marks[b]], PJ.intrinsics(cam), PJ.qvec2rotmat(qvec[row]), tvec[row], cam[1], cam[2])
        n = int(mask.sum())
        assert n_union[b] == len(marks[b]) and n_cand[b] == n, (b, n_union[b], n_cand[b], n)
        assert np.array_equal(cand_pt[b, :n], marks[b][mask]), b
        assert np.abs(cand_uv[b, :, :n] - np.stack([u[mask], v[mask]])).max() <= 1e-9, b
        # survivors and drop-outs in every chunk of 1024 candidates, so every chunk moves rows
        for c0 in range(0, len(marks[b]), 1024):
            assert mask[c0:c0 + 1024].any() and not mask[c0:c0 + 1024].all(), (b, c0)


@pytest.fixture(scope="module")
def match_cases():
    """The crafted inputs and their dense expectation, computed once."""
    out = []
    for roll in (0, 4):
        case = PJ.match_case(MATCH_SEED, roll)
        out.append((case, PJ.match_expected(case)))
    return out


def _run_match(case, dev):
    from pram_amd import ops
    tables = {"pt_desc": _t(case["pt_desc"], torch.float32, dev), "n_points": case["pt_desc"].shape[0]}
    args = (_t(case["kpts"], torch.float32, dev), _t(case["desc"], torch.float32, dev), _t(case["counts"], torch.int32, dev),
            _t(case["cand_pt"], torch.int32, dev), _t(case["cand_uv"], torch.float64, dev), _t(case["n_cand"], torch.int32, dev), tables, case["threshold"])
    return [x.cpu().numpy() for x in ops.projref_match(*args)]


def test_match_against_dense(dev, match_cases):
    """pram_projref_match against the dense formula: keypoint counts 0, 1, 63, 64, 65, 192 (the padded width) and 150, candidate
    counts 0, 1, 2, 63, 64, 65 and 3000 (two full chunks of 64 and many more, plus a remainder), keypoints with 0, 1, 2 and many
    in-range candidates.  best and accept exact, d0 / d1 within 1e-4 where finite, infinities exactly where fewer than one / two
    candidates are in range; padded keypoints come back empty; twice, bit-equal."""
    seen, pairs = set(), set()
    for case, want in match_cases:
        got = _run_match(case, dev)
        again = _run_match(case, dev)
        for g, a in zip(got, again):
            assert np.array_equal(g.view(np.uint8), a.view(np.uint8))
        best, d0, d1, accept = got
        for b, dm in enumerate(want):
            m, n = int(case["counts"][b]), int(case["n_cand"][b])
            pairs.add((m, n))
            wb, w0, w1, wa = PJ.gated_view(dm)
            assert np.array_equal(best[b, :m], wb), (b, m, n)
            assert np.array_equal(accept[b, :m], wa), (b, m, n, np.nonzero(accept[b, :m] != wa)[0])
            for g, w in ((d0[b, :m], w0), (d1[b, :m], w1)):
                assert np.array_equal(np.isinf(g), np.isinf(w)) and (g[np.isinf(g)] > 0).all(), (b, m, n)
                fin = np.isfinite(w)
                assert not fin.any() or np.abs(g[fin] - w[fin]).max() < D_BAR, (b, m, n)
            assert (best[b, m:] == -1).all() and np.isposinf(d0[b, m:]).all() and np.isposinf(d1[b, m:]).all() and not accept[b, m:].any()
            seen.update(f"in{min(int(k), 3)}" for k in dm["n_in"])
            if n >= 2 and m:
                seen.update({"accepted"} if wa.any() else set())
                seen.update({"ratio_rejected"} if ((dm["n_in"] >= 2) & (wa == 0)).any() else set())
    print(f"match: pairs {sorted(pairs)}, {sorted(seen)}")
    assert seen == {"in0", "in1", "in2", "in3", "accepted", "ratio_rejected"}
    assert {m for m, _ in pairs} == set(PJ.MATCH_COUNTS) and {n for _, n in pairs} == set(PJ.MATCH_CANDS) and (192, 3000) in pairs


def test_match_on_the_projrefine_fixture(dev, golden):
    """The fixture of tests/test_edges.py::test_hip_projection_refinement (what the imported reference handed its solver for 1500
    points and 600 keypoints): the fused kernel accepts the golden's keypoints with the golden's points, and agrees with the
    dense path recognition_post.refine_matches_by_projection on the same candidates."""
    from pram_amd import ops
    from pram_amd.localization import recognition_post as P
    from tests.test_edges import _projrefine_inputs
    g = golden("projrefine_n1500_m600")
    a = _projrefine_inputs(g)
    f64 = lambda x: _t(np.asarray(x, dtype=np.float64), torch.float64, dev)
    _, mask, keep, uvk, count = ops.project_points(f64(a["xyzs"]).reshape(-1, 3), f64(a["K"]), f64(a["Tcw"]), float(a["im_w"]), float(a["im_h"]))
    n = int(count.item())
    assert np.array_equal(mask.cpu().numpy().astype(bool), g["point_mask"].astype(bool))
    kp = _t(np.asarray(a["q_kpts"], dtype=np.float32)[:, :2], torch.float32, dev)[None].contiguous()
    qd = _t(a["q_descs"], torch.float32, dev)[None].contiguous()
    m = qd.shape[1]
    tables = {"pt_desc": _t(a["descs"], torch.float32, dev), "n_points": a["descs"].shape[0]}
    best, d0, d1, accept = ops.projref_match(kp, qd, _t(np.array([m]), torch.int32, dev), keep[None].contiguous(), uvk[None].contiguous(),
                                             _t(np.array([n]), torch.int32, dev), tables, a["threshold"])
    ok = accept[0].bool()
    kpt_ids = torch.nonzero(ok).flatten().cpu().numpy()
    pt_ids = keep[best[0][ok].long()].cpu().numpy()
    assert np.array_equal(kpt_ids, g["matched_keypoint_ids"]) and np.array_equal(pt_ids, g["matched_point_ids"])
    r = P.refine_matches_by_projection(a["q_kpts"], a["q_descs"], a["xyzs"], a["descs"], a["K"], a["Tcw"], a["im_w"], a["im_h"], a["threshold"])
    assert np.array_equal(kpt_ids, r["matched_keypoint_ids"].cpu().numpy()) and np.array_equal(pt_ids, r["matched_point_ids"].cpu().numpy())
    dense = r["dists"].cpu().numpy()
    got = np.stack([d0[0].cpu().numpy(), d1[0].cpu().numpy()], 1)
    both = np.isfinite(got) & (dense < 100)
    assert np.array_equal(np.isfinite(got), dense < 100) and np.abs(got[both] - dense[both]).max() < D_BAR
    print(f"projrefine fixture: {n} candidates, {len(kpt_ids)} of {m} keypoints accepted")


def test_correspond_exact(dev):
    """Crafted accept / best: nothing accepted (count 0), everything accepted, every other keypoint, a chunk boundary at 256;
    every field bit-equal to numpy's boolean indexing, rows beyond the count keep the sentinel they were filled with."""
    from pram_amd import ops
    rng = np.random.default_rng(3)
    n_points, N, cap = 700, 600, 500
    counts = np.array([600, 600, 257, 256, 0, 300, 1], np.int32)
    B = len(counts)
    n_cand = np.array([500, 500, 77, 2, 500, 0, 1], np.int32)
    accept = (rng.uniform(0, 1, (B, N)) < 0.5).astype(np.uint8)
    accept[0], accept[1] = 0, 1
    best = np.stack([rng.integers(0, max(int(c), 1), N) for c in n_cand]).astype(np.int32)
    accept[5] = 0      # no candidates: the match kernel accepts nothing there
    cand_pt = np.stack([np.sort(rng.permutation(n_points)[:cap]) for _ in range(B)]).astype(np.int32)
    tables = {"pt_ids": _t(np.sort(rng.permutation(10 ** 6)[:n_points]) * 1001 + 5, torch.int64, dev), "pt_xyz": _t(rng.standard_normal((n_points, 3)), torch.float64, dev),
              "pt_sid": _t(rng.integers(-1, 50, n_points), torch.int32, dev), "n_points": n_points}
    kpts = rng.uniform(0, 640, (B, N, 2)).astype(np.float32)
    fill = lambda: {"matched_keypoint_ids": torch.full((B, N), -7, dtype=torch.int64, device=dev), "matched_keypoints": torch.full((B, N, 2), -7.0, device=dev),
                    "matched_point3D_ids": torch.full((B, N), -7, dtype=torch.int64, device=dev),
                    "matched_xyzs": torch.full((B, N, 3), -7.0, dtype=torch.float64, device=dev),
                    "matched_sids": torch.full((B, N), -7, dtype=torch.int32, device=dev), "count": torch.full((B,), -7, dtype=torch.int32, device=dev)}
    args = (_t(accept, torch.uint8, dev), _t(best, torch.int32, dev), _t(counts, torch.int32, dev), _t(kpts, torch.float32, dev), _t(cand_pt, torch.int32, dev),
            _t(n_cand, torch.int32, dev), tables)
    out = {k: v.cpu().numpy() for k, v in ops.projref_correspond(*args, out=fill()).items()}
    pid, xyz, sid = tables["pt_ids"].cpu().numpy(), tables["pt_xyz"].cpu().numpy(), tables["pt_sid"].cpu().numpy()
    for b in range(B):
        keep = np.nonzero(accept[b, :counts[b]])[0]
        pts = cand_pt[b, best[b, keep]]
        n = len(keep)
        assert out["count"][b] == n, (b, out["count"][b], n)
        assert np.array_equal(out["matched_keypoint_ids"][b, :n], keep) and np.array_equal(out["matched_keypoints"][b, :n], kpts[b, keep])
        assert np.array_equal(out["matched_point3D_ids"][b, :n], pid[pts]) and np.array_equal(out["matched_sids"][b, :n], sid[pts])
        assert np.array_equal(out["matched_xyzs"][b, :n].view(np.uint8), xyz[pts].view(np.uint8))
        for k in ("matched_keypoint_ids", "matched_keypoints", "matched_point3D_ids", "matched_xyzs", "matched_sids"):
            assert (out[k][b, n:] == -7).all(), (b, k, "rows beyond the count were written")
    assert out["count"][0] == 0 and out["count"][1] == 600 and out["count"][4] == 0 and out["count"][5] == 0
    again = ops.projref_correspond(*args)
    assert np.array_equal(again["count"].cpu().numpy(), out["count"]) and again["matched_xyzs"].shape == (B, N, 3)


@pytest.fixture(scope="module")
def pscene(dev):
    map_, queries, planted, located = PJ.projection_scene()
    store = _store(map_, dev, covisibility_frame=RR.COVIS)
    per_entry = [queries[l["query"]] if l is not None else queries[4] for l in located]
    feats, _ = CR.batch_features(per_entry, dev)
    cams = [planted[l["query"]]["cam"] if l is not None else planted[4]["cam"] for l in located]
    return {"map": map_, "queries": per_entry, "planted": planted, "located": located, "store": store, "features": feats, "cams": cams,
            "graph": RR.covisibility_graph(map_, RR.COVIS), "table": PJ.point_table(map_), "state": _state(located, store, dev),
            "enable": [bool(l["enable"]) if l is not None else True for l in located]}


def _refine(s, **kw):
    from pram_amd.localization.refine import refine_by_projection
    return refine_by_projection(s["features"], s["state"], s["store"], s["cams"], threshold=PJ.THRESHOLD, enable=s["enable"], **POSE, **kw)


def test_public_call(pscene, dev):
    """refine_by_projection on projection_scene (seven batch entries over covisible_scene's five queries; entry 0's reference frame
    is not in its own list): the matched lists are bit-equal to the restatement's, which uses the dense formula; n_union and
    n_projected are its counts; the distances agree within 1e-4; the pose equals pose_ref.estimate_pose on the device's own lists
    with p = b inside 4.12's bars; the frame vote equals the restatement's; entries with 64 matches or more stand within
    1 degree / 0.5 m of the planted camera; the entry that is not located and the disabled one come back None.

    Matches handed to the solver (seed 7, threshold 8): 126, 82, 53, 8, 126 (entries 0 .. 4; entry 6, disabled, would have 82).
    Query 2 has 64 keypoints, 52 of them planted, so it cannot reach 64 matches: the three entries that do are 0, 1 and 4.
    Inliers / matches on the MI355X (printed, asserted only through the equality with the restatement): 121 / 126, 81 / 82, 52 / 53,
    8 / 8, 120 / 126; the refined poses of entries 0, 1, 4 stand 0.17, 0.36, 0.11 degrees and 1.6, 2.6, 3.5 cm from the planted cameras
    (the planted localisations: 0.19, 0.31, 0.12 degrees, 2.0, 4.4, 2.7 cm); qvec deviates from pose_ref.estimate_pose by at most
    2.2e-12, tvec by 4.9e-12 relative."""
    s = pscene
    res = _refine(s)
    n_big = 0
    for b, (l, x) in enumerate(zip(s["located"], res)):
        if l is None or not l["enable"]:
            assert x is None, b
            continue
        cam = s["cams"][b]
        holder = {}

        def solver(k, xyz):
            holder["ref"] = PR.estimate_pose(k, xyz, cam, threshold=PJ.THRESHOLD, trials=POSE["trials"], refine_iters=POSE["refine_iters"], seed=POSE["seed"], p=b)
            return {"success": holder["ref"]["success"], "inliers": holder["ref"]["inliers"]}
        w = PJ.refine_by_projection(s["queries"][b], s["map"], l, cam, solver, threshold=PJ.THRESHOLD, covisibility_frame=RR.COVIS, graph=s["graph"],
                                    table=s["table"])
        ref = holder["ref"]
        assert x["n_union"] == len(w["union"]) and x["n_projected"] == len(w["cand"]), (b, x["n_union"], x["n_projected"])
        for k in ("matched_keypoints", "matched_keypoint_ids", "matched_xyzs", "matched_point3D_ids", "matched_sids"):
            g = x[k].cpu().numpy()
            ww = np.ascontiguousarray(w[k]).astype(g.dtype)
            assert g.shape == ww.shape and np.array_equal(g.view(np.uint8), ww.view(np.uint8)), (b, k, g.shape, ww.shape)
        _, w0, w1, _ = PJ.gated_view(w["dm"])
        dists = x["dists"].cpu().numpy()
        assert dists.shape == (s["queries"][b]["count"], 2)
        for g, ww in ((dists[:, 0], w0), (dists[:, 1], w1)):
            assert np.array_equal(np.isinf(g), np.isinf(ww)) and np.abs(g[np.isfinite(ww)] - ww[np.isfinite(ww)]).max(initial=0.0) < D_BAR, b
        n = len(w["matched_keypoint_ids"])
        assert x["success"] == ref["success"] and x["num_inliers"] == ref["num_inliers"], (b, x["num_inliers"], ref["num_inliers"])
        assert np.array_equal(x["inliers"].cpu().numpy(), ref["inliers"]), b
        dq = dt = 0.0
        if ref["success"]:
            dq = float(np.abs(x["qvec"] - ref["qvec"]).max())
            dt = float(np.abs(x["tvec"] - ref["tvec"]).max() / (1.0 + np.abs(ref["tvec"]).max()))
        e0 = PR.pose_errors(PJ.qvec2rotmat(l["qvec"]), l["tvec"], s["planted"][l["query"]]["R"], s["planted"][l["query"]]["t"])
        print(f"projection: entry {b} (query {l['query']}, frame {l['reference_frame_id']}): union {x['n_union']}, projected {x['n_projected']}, inliers "
              f"{x['num_inliers']}/{n}, success {x['success']}, dq {dq:.2e} dt {dt:.2e}, new frames {x['refinement_reference_frame_ids']}; "
              f"the localisation stood {e0[0]:.4f} deg, {e0[1]:.4f} m from the planted camera")
        assert dq <= E2E_Q_BAR and dt <= E2E_T_BAR, (b, dq, dt)
        assert x["refinement_reference_frame_ids"] == list(w["refinement_reference_frame_ids"]), (b, x["refinement_reference_frame_ids"])
        assert x["reference_frame_id"] == w["reference_frame_id"]
        if n >= 64:
            n_big += 1
            assert x["success"]
            er, ec = PR.pose_errors(PR.qvec_to_rot(x["qvec"]), x["tvec"], s["planted"][l["query"]]["R"], s["planted"][l["query"]]["t"])
            print(f"projection: entry {b} refined: {er:.4f} deg, {ec:.4f} m from the planted camera")
            assert er < 1.0 and ec < 0.5
    assert n_big >= 3
    # device_cameras' result needs image_sizes; with them the result is the same
    from pram_amd.localization import pose
    from pram_amd.localization.refine import image_size_table, refine_by_projection
    resident = pose.device_cameras(s["cams"], dev)
    with pytest.raises(ValueError):
        refine_by_projection(s["features"], s["state"], s["store"], resident, threshold=PJ.THRESHOLD, **POSE)
    again = refine_by_projection(s["features"], s["state"], s["store"], resident, threshold=PJ.THRESHOLD, enable=s["enable"], image_sizes=image_size_table(s["cams"]),
                                 **POSE)
    for x, y in zip(res, again):
        _same(x, y)
    # the lists cut to one frame: entry 0's list no longer holds its reference frame either way, the union shrinks
    short = _refine(s, covisibility_frame=1)
    g1 = RR.covisibility_graph(s["map"], 1)
    for b, l in enumerate(s["located"]):
        if l is not None and l["enable"]:
            assert short[b]["n_union"] == len(PJ.union_points(s["map"], g1, l["reference_frame_id"], s["table"])) < res[b]["n_union"], b


def _same(x, y):
    assert (x is None) == (y is None)
    if x is None:
        return
    assert set(x) == set(y)
    for k, v in x.items():
        if torch.is_tensor(v):
            assert torch.equal(v, y[k]), k
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, y[k]), k
        else:
            assert v == y[k], k


def test_determinism(pscene):
    a, b = _refine(pscene), _refine(pscene)
    assert any(x is not None for x in a)
    for x, y in zip(a, b):
        _same(x, y)


@pytest.fixture(scope="module")
def scene(dev):
    m, qs, planted = RR.covisible_scene()
    store = _store(m, dev, covisibility_frame=RR.COVIS)
    feats, seg = CR.batch_features(qs, dev)
    return {"map": m, "queries": qs, "planted": planted, "cams": [p["cam"] for p in planted], "store": store, "features": feats, "seg": seg}


def _same_matching(x, y):
    assert (x is None) == (y is None)
    if x is not None:
        TGR._same_refinement({k: v for k, v in x.items() if k != "method"}, y)


def test_localize_and_refine_methods(scene, dev):
    """The default equals refine_by_matching called on the localisation's state, bit for bit; 'projection' sends a tracked query
    with projection_min_inliers or more to refine_by_projection and every other located query to refine_by_matching, each equal
    to the direct call with that enable mask; an unknown method raises."""
    from pram_amd.localization import pose
    from pram_amd.localization.refine import localize_and_refine, refine_by_matching, refine_by_projection
    net = TGR._gml(dev)
    s, LOC = scene, TGR.LOC
    args = (s["features"], s["seg"], s["store"], net, s["cams"])
    kw = dict(LOC, overlap_ratio=0.5, min_inlier_ratio=0.01, refine_iters=20)
    loc, state = pose._localize(*args, **kw)
    rkw = dict(threshold=LOC["threshold"], trials=LOC["trials"], seed=LOC["seed"])
    direct = refine_by_matching(s["features"], state, s["store"], net, s["cams"], **rkw)
    default = localize_and_refine(*args, **LOC)
    TGR._same_localisation(loc, default)
    for r, y in zip(default, direct):
        _same_matching(r["refinement"], y)
        assert r["refinement"] is None or r["refinement"]["method"] == "matching"
    inl = [r["num_inliers"] if r["success"] else None for r in loc]
    tracked = [b for b, r in enumerate(loc) if r["success"] and r["tracking_status"]]
    assert len(tracked) >= 2
    bar = sorted(loc[b]["num_inliers"] for b in tracked)[-2]      # the two strongest tracked queries go to projection
    strong = [bool(r["success"] and r["tracking_status"] and r["num_inliers"] >= bar) for r in loc]
    weak = [bool(r["success"]) and not st for r, st in zip(loc, strong)]
    print(f"method switch: inliers {inl}, status {[r['tracking_status'] for r in loc]}, projection_min_inliers {bar}: projection {strong}, matching {weak}")
    assert sum(strong) >= 2 and sum(weak) >= 1 and any(loc[b]["tracking_status"] for b in range(len(loc)) if weak[b]) and bar < 64
    res = localize_and_refine(*args, **LOC, refinement_method="projection", projection_min_inliers=bar)
    TGR._same_localisation(loc, res)
    by_proj = refine_by_projection(s["features"], state, s["store"], s["cams"], enable=strong, **rkw)
    by_match = refine_by_matching(s["features"], state, s["store"], net, s["cams"], enable=weak, **rkw)
    for b, r in enumerate(res):
        x = r["refinement"]
        if strong[b]:
            assert x["method"] == "projection" and "n_projected" in x and "slots" not in x
            _same({k: v for k, v in x.items() if k != "method"}, by_proj[b])
            print(f"method switch: query {b} by projection: inliers {r['num_inliers']}/{r['matched_keypoints'].shape[0]} -> {x['num_inliers']}/"
                  f"{x['matched_keypoints'].shape[0]}, success {x['success']}")
        elif weak[b]:
            assert x["method"] == "matching" and "slots" in x
            _same_matching(x, by_match[b])
        else:
            assert x is None
    # the default bar: nobody reaches 64 inliers here... or everybody goes where multimap3d.py:245-255 sends them
    full = localize_and_refine(*args, **LOC, refinement_method="projection")
    for b, r in enumerate(full):
        want = None if not loc[b]["success"] else ("projection" if loc[b]["tracking_status"] and loc[b]["num_inliers"] >= 64 else "matching")
        assert (r["refinement"]["method"] if r["refinement"] is not None else None) == want, b
    with pytest.raises(NotImplementedError):
        localize_and_refine(*args, **LOC, refinement_method="bundle")


def test_ctypes_entries(hip_lib, dev):
    """The four entries through ctypes alone on hand-written tables, with every error status."""
    L = hip_lib
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=dev)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # three frames of 3, 2, 2 rows; covisible lists: frame 0 -> [1], frame 1 -> [], frame 2 -> [2, 0]
    frame_off, covis_off, covis_frames = i32([0, 3, 5, 7]), i32([0, 1, 1, 3]), i32([1, 2, 0])
    point3d_ids, pt_ids = i64([11, -1, 15, 12, 99, 15, 17]), i64([11, 12, 15, 17])
    # query 0 kept candidate 1 (frame 0: not in its own list), query 1 kept candidate 0 (frame 2), query 2 is not located
    chosen = i32([[1, 1, 1], [0, 1, 0], [-1, -1, -1]])
    loc_plan = torch.zeros(10, 6, dtype=torch.int32, device=dev)
    loc_plan[2] = i32([1, 0, 2, 1, 0, 0])
    bitmap, ref = i32([77, 77, 77]), i32([-9, -9, -9])

    def run_mark(n_cov=2, chosen_=chosen, ids=point3d_ids, n_points=4, enable=None, bitmap_=bitmap):
        return L.pram_projref_mark(p(chosen_), p(loc_plan), p(enable), p(frame_off), p(covis_off), p(covis_frames), C.c_void_p(ids.data_ptr()), p(pt_ids), 3, 2, n_cov,
                                   3, 3, 7, n_points, p(bitmap_), p(ref), st)
    assert run_mark() == 0
    # query 0: frame 1 (12; 99 unknown) and frame 0 itself (11, 15; -1 skipped) -> bits 0, 1, 2; query 1: frames 2 and 0 -> 11, 15, 17 -> bits 0, 2, 3
    assert bitmap.tolist() == [0b0111, 0b1101, 0] and ref.tolist() == [0, 2, -1]
    assert run_mark(enable=i32([0, 1, 1])) == 0 and bitmap.tolist() == [0, 0b1101, 0] and ref.tolist() == [-1, 2, -1]
    assert run_mark(n_cov=1) == 0 and bitmap.tolist() == [0b0111, 0b1100, 0]      # query 1's list cut to [2]: 15, 17
    assert run_mark() == 0
    # projection: identity pose, PINHOLE f = 100, centre (50, 40), image 100 x 80
    pt_xyz = f64([[0.0, 0.0, 2.0], [1.5, 0.0, 2.0], [0.0, 0.0, -1.0], [-0.25, 0.2, 1.0]])      # 12 leaves on the right, 15 is behind
    qvec, tvec = f64([[9, 9, 9, 9], [1, 0, 0, 0], [1, 0, 0, 0], [9, 9, 9, 9], [9, 9, 9, 9], [9, 9, 9, 9]]), torch.zeros(6, 3, dtype=torch.float64, device=dev)
    cam_model, cam_params, sizes = i32([1, 1, 1]), f64([[100, 100, 50, 40, 0, 0, 0, 0]] * 3), i32([[100, 80]] * 3)
    cap = 4
    cand_pt, cand_uv, n_union, n_cand = i32(np.full((3, cap), -9)), f64(np.full((3, 2, cap), -9.0)), i32([-9] * 3), i32([-9] * 3)

    def run_project(cap=cap, n_points=4, xyz=pt_xyz, uv=cand_uv):
        return L.pram_projref_project(p(bitmap), n_points, p(xyz), p(chosen), p(qvec), p(tvec), p(cam_model), p(cam_params), p(sizes), 3, 2, cap, p(cand_pt),
                                      C.c_void_p(uv.data_ptr()), p(n_union), p(n_cand), st)
    assert run_project() == 0
    assert n_union.tolist() == [3, 3, 0] and n_cand.tolist() == [1, 2, 0]
    assert cand_pt[0, :1].tolist() == [0] and cand_uv[0, :, 0].tolist() == [50.0, 40.0]
    assert cand_pt[1, :2].tolist() == [0, 3] and cand_uv[1, :, :2].tolist() == [[50.0, 25.0], [40.0, 60.0]]
    # matching: two keypoints per query; descriptors: unit vectors e0 / e1
    e = torch.zeros(4, 128, device=dev)
    e[0, 0], e[1, 1], e[2, 2], e[3, 0] = 1.0, 1.0, 1.0, 0.6
    e[3, 1] = 0.8
    q_kpts = torch.tensor([[[50.0, 40.0], [90.0, 70.0]], [[30.0, 50.0], [26.0, 59.0]], [[0.0, 0.0], [0.0, 0.0]]], device=dev)
    q_desc = torch.zeros(3, 2, 128, device=dev)
    q_desc[:, :, 0] = 1.0
    counts = i32([2, 2, 2])
    best, d0, d1, accept = i32(np.full((3, 2), -9)), torch.full((3, 2), -9.0, device=dev), torch.full((3, 2), -9.0, device=dev), torch.full((3, 2), 9, dtype=torch.uint8, device=dev)

    def run_match(threshold=8.0, n=2, desc=q_desc, n_points=4, cap=cap):
        return L.pram_projref_match(p(q_kpts), C.c_void_p(desc.data_ptr()), p(counts), 3, n, p(cand_pt), p(cand_uv), p(n_cand), cap, p(e), n_points,
                                    C.c_double(threshold), p(best), p(d0), p(d1), p(accept), st)
    assert run_match() == 0
    # query 0 has one candidate: topk(k = 2) has nothing to take, nothing is accepted though keypoint 0 sits on it
    assert best[0].tolist() == [0, -1] and accept[0].tolist() == [0, 0] and d0[0, 0].item() == pytest.approx(1e-3, abs=1e-6) and torch.isinf(d1[0]).all()
    # query 1, range 16: keypoint 0 at (30, 50) is 22.4 from candidate 0 and 11.2 from candidate 1: one in range -> accepted;
    # keypoint 1 at (26, 59) is 30.6 and 1.4 away: one in range as well
    assert best[1].tolist() == [1, 1] and accept[1].tolist() == [1, 1] and torch.isinf(d1[1]).all()
    assert d0[1, 0].item() == pytest.approx(np.sqrt(2 - 2 * 0.6 + 1e-6), abs=1e-6)
    assert run_match(threshold=12.0) == 0      # range 24: both candidates in range of keypoint 0; 0.0010 / 0.894 passes the ratio test
    assert best[1].tolist() == [0, 1] and accept[1].tolist() == [1, 1] and d1[1, 0].item() == pytest.approx(np.sqrt(2 - 2 * 0.6 + 1e-6), abs=1e-6)
    assert best[2].tolist() == [-1, -1] and accept[2].tolist() == [0, 0]
    # correspondences
    pt_sid = i32([5, 6, 7, 8])
    m_ids, m_kp, m_p3, m_xyz, m_sid, m_cnt = i64(np.full((3, 2), -5)), torch.full((3, 2, 2), -5.0, device=dev), i64(np.full((3, 2), -5)), \
        f64(np.full((3, 2, 3), -5.0)), i32(np.full((3, 2), -5)), i32([-5] * 3)

    def run_cor(n=2, xyz_out=m_xyz, acc=accept, n_points=4):
        return L.pram_projref_correspond(p(acc), p(best), p(counts), p(q_kpts), 3, n, p(cand_pt), p(n_cand), cap, p(pt_ids), p(pt_xyz), p(pt_sid), n_points, p(m_ids),
                                         p(m_kp), p(m_p3), C.c_void_p(xyz_out.data_ptr()), p(m_sid), p(m_cnt), st)
    assert run_cor() == 0
    assert m_cnt.tolist() == [0, 2, 0] and m_ids[1].tolist() == [0, 1] and m_p3[1].tolist() == [11, 17] and m_sid[1].tolist() == [5, 8]
    assert torch.equal(m_xyz[1], pt_xyz[[0, 3]]) and torch.equal(m_kp[1], q_kpts[1]) and m_ids[0].tolist() == [-5, -5]
    torch.cuda.synchronize()
    # error statuses: nothing is launched
    E_ARG = -1
    assert run_mark(n_cov=0) == E_ARG and b"n_cov" in L.pram_last_error()
    assert run_mark(chosen_=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_mark(n_points=0) == E_ARG and b"n_points" in L.pram_last_error()
    assert run_mark(ids=point3d_ids.view(torch.int32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
    assert run_mark(bitmap_=None) == E_ARG
    assert run_project(cap=0) == E_ARG and b"cap" in L.pram_last_error()
    assert run_project(n_points=0) == E_ARG
    assert run_project(xyz=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_project(uv=cand_uv.view(torch.float32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
    assert run_match(threshold=0.0) == E_ARG and b"threshold" in L.pram_last_error()
    assert run_match(threshold=float("nan")) == E_ARG and run_match(threshold=float("inf")) == E_ARG
    assert run_match(n=-1) == E_ARG and run_match(cap=0) == E_ARG and run_match(n_points=0) == E_ARG
    assert run_match(desc=q_desc.view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
    assert run_cor(n=-1) == E_ARG and run_cor(n_points=0) == E_ARG
    assert run_cor(acc=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_cor(xyz_out=m_xyz.view(torch.float32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
    assert bitmap.tolist() == [0b0111, 0b1101, 0] and m_cnt.tolist() == [0, 2, 0]
