"""GPU: localisation against retrieved database frames (pram_amd.localization.retrieval, csrc/retrieval.hip) against the numpy
restatement tests/retrieval_ref.py: the four kernels on their own, the public calls stage by stage, and the C entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import helpers as H
from tests import pose_ref as PR
from tests import refine_ref as RR
from tests import retrieval_ref as TR

pytestmark = pytest.mark.gpu

E2E_Q_BAR, E2E_T_BAR = 1e-8, 2e-8      # the bars of tests/test_gpu_pose.py for the same kernels
COR_KEYS = ("matched_keypoint_ids", "matched_keypoints", "matched_ref_keypoints", "matched_point3D_ids", "matched_xyzs", "matched_sids")
COR_DTYPES = (torch.int64, torch.float32, torch.float32, torch.int64, torch.float64, torch.int32)
COR_TAILS = ((), (2,), (2,), (), (3,), ())
# min_inlier_ratio 0.6: GML on the synthetic weights matches a handful of query 3's keypoints to points it does not see (8 rows survive
# obs_th 3, 4 of them agree with some pose); the pose stage refuses such a support, and query 3 takes the failure path
POSE = dict(threshold=4.0, trials=300, seed=4, min_inlier_ratio=0.6)
COVIS_K = 3


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gml(dev):
    from pram_amd.nets.gml import GML
    g = GML({})
    g.load_state_dict(H.gml_sd(), strict=True)
    return g.to(dev).eval()


def _real(q):
    return {k: (v[:q["count"]] if isinstance(v, np.ndarray) else v) for k, v in q.items() if k != "padded"}


@pytest.fixture(scope="module")
def scene(dev):
    from pram_amd.localization.retrieval import DatabaseStore
    m, qs, planted = RR.covisible_scene()
    m = dict(m, poses={fid: (np.array([1.0, 0.0, 0.0, 0.0]) * (1 + i), np.arange(3.0) + i) for i, fid in enumerate(RR.frame_ids(m))})
    store = DatabaseStore(m["frames"], m["seg_ref_frame_ids"], 0, device=dev, covisibility_frame=RR.COVIS, poses=m["poses"])
    feats, _ = CR.batch_features(qs, dev)
    return {"map": m, "queries": [_real(q) for q in qs], "planted": planted, "cams": [p["cam"] for p in planted], "store": store, "features": feats,
            "net": _gml(dev)}


def _crafted_map(seed=5, n_frames=12, n_points=300):
    """Twelve frames of 5 .. 30 rows over 300 points whose frame lists are given (1 .. 6 entries, duplicates among them, some
    naming frames the store does not hold); rows with id -1 and with ids outside the point table; frame 7 has rows of -1 only."""
    rng = np.random.default_rng(seed)
    ids = (rng.permutation(5000)[:n_points] * 7 + 3).astype(np.int64)
    p2f = {int(i): (50 + rng.integers(0, n_frames + 2, rng.integers(1, 7))).tolist() for i in ids}
    frames = []
    for f in range(n_frames):
        n = int(rng.integers(5, 31))
        pid = rng.choice(np.concatenate([ids, [-1, -1, 1, 2]]), n)
        if f == 7:
            pid[:] = -1
        frames.append({"id": 50 + f, "keypoints": np.zeros((n, 3), np.float32), "descriptors": np.zeros((n, 128), np.float32), "xyzs": np.zeros((n, 3)),
                       "point3D_ids": pid.astype(np.int64), "width": 640, "height": 480})
    return {"frames": frames, "seg_ref_frame_ids": {}, "start_sid": 0, "point3D_frame_ids": p2f}


def _expected_plan(table, counts, enable, store):
    from pram_amd import ops
    B, n_db = table.shape
    plan = np.zeros((ops.CAND_PLAN_COLS, B * n_db), dtype=np.int32)
    for b in range(B):
        for j in range(n_db):
            g = int(table[b, j])
            g = g if 0 <= g < store.n_frames else -1
            nv = int(store.valid_off[g + 1] - store.valid_off[g]) if g >= 0 else 0
            live = g >= 0 and nv > 0 and counts[b] > 0 and (enable is None or enable[b] != 0)
            plan[:, b * n_db + j] = [b, -1, g if live else -1, 0, counts[b] if live else 0, nv if live else 0, -1, int(store.frame_off[g]) if live else 0,
                                     int(store.valid_off[g]) if live else -1, j]
    return plan


def test_plan_exact(scene, dev):
    """Every column against a table written in numpy: a -1 slot, slots at and beyond n_frames, a frame whose rows are all -1,
    counts 0 and below, enable 0, n_db 1."""
    from pram_amd import ops
    from pram_amd.localization.retrieval import DatabaseStore
    two = DatabaseStore([{"keypoints": np.zeros((4, 3), np.float32), "descriptors": np.zeros((4, 128), np.float32), "xyzs": np.zeros((4, 3)),
                          "point3D_ids": np.full(4, -1, np.int64), "width": 8, "height": 8},
                         {"keypoints": np.zeros((3, 3), np.float32), "descriptors": np.zeros((3, 128), np.float32), "xyzs": np.zeros((3, 3)),
                          "point3D_ids": np.array([9, -1, 4], np.int64), "width": 8, "height": 8}], device=dev)
    assert two.valid_off.tolist() == [0, 0, 2] and two.valid_rows.tolist() == [4, 6]
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)
    cases = [(scene["store"], [[1, 0, 2, 6], [5, 4, 3, -1], [7, -1, -1, -1], [8, 9, 100, 7], [0, 1, 2, 3], [3, 3, -5, 3]], [150, 100, 64, 10, 0, -2], [1, 1, 0, 1, 1, 1]),
             (scene["store"], [[7], [8], [-1], [0]], [5, 5, 5, 0], [1, 1, 1, 1]),
             (two, [[0, 1], [1, 0], [1, 2]], [6, 6, 6], [1, 0, 1])]
    for store, table, counts, enable in cases:
        table = np.array(table, dtype=np.int32)
        for en in (None, enable):
            got = ops.retr_plan(i32(table), i32(counts), store.tables(dev), None if en is None else i32(en)).cpu().numpy()
            want = _expected_plan(table, counts, en, store)
            assert np.array_equal(got, want), (table.tolist(), en, got.tolist(), want.tolist())
    p = dict(zip(ops.CAND_PLAN_FIELDS, _expected_plan(np.array(cases[2][1], dtype=np.int32), cases[2][2], None, two)))
    assert p["lens1"].tolist() == [0, 2, 2, 0, 2, 0] and p["sel_off"].tolist() == [-1, 0, 0, -1, 0, -1] and p["frame"].tolist() == [-1, 1, 1, -1, 1, -1]


def _random_cor(rng, P, t, counts, dev, p3d_pool):
    """pram_cand_correspond-shaped buffers with every bit random (xyz: random 64-bit words read as float64), point ids from a pool"""
    out = {}
    for k, dt, tail in zip(COR_KEYS, COR_DTYPES, COR_TAILS):
        nbytes = int(np.prod((P, t) + tail)) * torch.empty(0, dtype=dt).element_size()
        out[k] = torch.from_numpy(rng.integers(0, 256, nbytes, dtype=np.uint8)).view(dt).reshape((P, t) + tail).to(dev)
    out["matched_point3D_ids"] = torch.from_numpy(rng.choice(p3d_pool, (P, t))).to(dev)
    out["count"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    return out


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).reshape(-1).view(np.uint8)


def _sentinel(P, t, dev):
    out = {k: torch.from_numpy(np.full(int(np.prod((P, t) + tail)) * torch.empty(0, dtype=dt).element_size(), 0xA5, np.uint8)).view(dt).reshape((P, t) + tail).to(dev)
           for k, dt, tail in zip(COR_KEYS, COR_DTYPES, COR_TAILS)}
    out["count"] = torch.full((P,), -7, dtype=torch.int32, device=dev)
    return out


def test_filter_and_stack_exact(scene, dev):
    """Crafted lists, no matcher: per pair the kept rows bit-equal to numpy selection in order, rows beyond the count untouched;
    obs_th 0 and 3 (and 2, 5: nothing left); ids absent from the table; slots of 0 rows between full ones; more than 256 rows in a
    slot (the chunk loop).  The stack is pram_refine_merge's with init_on 0, whose cap (n_db + 1) * t0 no stack can exceed: a slot
    whose count word says t0 + 1 is cut to t0 by the filter, and every slot full gives n_db * t0 rows, the most a stack holds."""
    from pram_amd import ops
    from pram_amd.localization import retrieval as RT
    store = scene["store"]
    tables = store.tables(dev)
    rng = np.random.default_rng(12)
    n_db, t0 = 3, 300
    counts = [[300, 0, 300], [257, 1, 0], [0, 0, 0], [301, 300, 300], [64, 255, 256]]
    B = len(counts)
    pool = np.concatenate([store.pt_ids, np.array([-1, 1, 2, 10 ** 12, store.pt_ids.max() + 1])])
    cor = _random_cor(rng, B * n_db, t0, [c for row in counts for c in row], dev, pool)
    p3d = cor["matched_point3D_ids"].cpu().numpy()
    n_dropped = 0
    for obs_th in (0, 3, 2, 5, -1):
        out = ops.retr_filter(cor, tables, obs_th, out=_sentinel(B * n_db, t0, dev))
        sent = _sentinel(B * n_db, t0, dev)
        got_counts = out["count"].cpu().numpy()
        keeps = []
        for p in range(B * n_db):
            n = min(counts[p // n_db][p % n_db], t0)
            keep = np.nonzero((store.observations(p3d[p, :n]) >= obs_th) | (obs_th <= 0))[0]
            keeps.append(keep)
            n_dropped += n - len(keep)
            assert got_counts[p] == len(keep), (obs_th, p, got_counts[p], len(keep))
            idx = torch.from_numpy(keep).to(dev)
            for k in COR_KEYS:
                assert np.array_equal(_bits(out[k][p, :len(keep)]), _bits(cor[k][p][idx])), (obs_th, p, k)
                assert np.array_equal(_bits(out[k][p, len(keep):]), _bits(sent[k][p, len(keep):])), (obs_th, p, k, "rows beyond the count were written")
        if obs_th == 5:
            assert got_counts.sum() == 0
        if obs_th <= 0:
            assert got_counts.reshape(B, n_db).tolist() == [[min(c, t0) for c in row] for row in counts]
        stack = RT._stack(out, n_db)
        sc = stack["count"].cpu().numpy()
        assert stack["matched_sids"].shape[1] == (n_db + 1) * t0
        for b in range(B):
            want_src = np.concatenate([np.full(len(keeps[b * n_db + j]), j, np.int32) for j in range(n_db)])
            assert sc[b] == len(want_src) and np.array_equal(stack["matched_src"][b, :sc[b]].cpu().numpy(), want_src), (obs_th, b)
            for k in COR_KEYS:
                want = torch.cat([out[k][b * n_db + j, :len(keeps[b * n_db + j])] for j in range(n_db)])
                assert np.array_equal(_bits(stack[k][b, :sc[b]]), _bits(want)), (obs_th, b, k)
        if obs_th <= 0:
            assert sc[3] == n_db * t0 and sc[2] == 0 and sc[0] == 600
    assert n_dropped > 1000


def test_select_exact(dev):
    """One query per branch on a [B, 6] table, against the restatement's walk."""
    from pram_amd import ops
    rows = [  # (success, num_inliers, count)
        ([1] * 6, [60, 99, 0, 0, 0, 0], [20] * 6),                      # accepted at slot 0
        ([1] * 6, [30, 45, 40, 50, 99, 99], [9] * 6),                   # accepted at slot 3, larger ones behind it; the best moved 0, 1, 3
        ([1] * 6, [49, 20, 30, 50, 0, 0], [9] * 6),                     # accepted at slot 3; until then slot 0 was the best, by 1 under the bar
        ([1] * 6, [99, 50, 0, 0, 0, 0], [7, 8, 8, 8, 8, 8]),            # count 7 passed over, count 8 taken
        ([0] * 6, [99] * 6, [20] * 6),                                  # every slot failed
        ([1] * 6, [3, 10, 4, 10, 2, 1], [20] * 6),                      # best exactly min_best_inliers; the first of a tie
        ([1] * 6, [3, 9, 4, 9, 2, 1], [20] * 6),                        # one below
        ([1, 0, 1, 1, 1, 1], [20, 48, 30, 30, 29, 0], [20] * 6),        # a tie for best, the first wins; a failed slot with more
        ([1] * 6, [0] * 6, [0] * 6),                                    # all slots empty
        ([1] * 6, [-3, -1, 0, 0, 0, 0], [20] * 6),                      # nothing above 0: no best
    ]
    t = lambda i: torch.tensor([r[i] for r in rows], dtype=torch.int32, device=dev).reshape(-1).contiguous()
    got = ops.retr_select(t(0), t(1), t(2), 6, 50, 10).cpu().tolist()
    want = [list(TR.select(*r, 50, 10)) for r in rows]
    assert got == want, (got, want)
    assert want == [[0, 1, 0], [3, 1, 3], [3, 1, 3], [1, 1, 1], [-1, 0, -1], [1, 2, 1], [-1, 0, 1], [2, 2, 2], [-1, 0, -1], [-1, 0, -1]]
    got = ops.retr_select(t(0), t(1), t(2), 6, 45, 9).cpu().tolist()
    assert got == [list(TR.select(*r, 45, 9)) for r in rows] and got[1][0] == 1 and got[6] == [1, 2, 1]
    one = ops.retr_select(t(0)[:6].contiguous(), t(1)[:6].contiguous(), t(2)[:6].contiguous(), 1, 50, 10).cpu().tolist()      # n_db 1
    assert one == [[0, 1, 0], [0, 1, 0], [-1, 0, -1], [-1, 0, -1], [-1, 0, -1], [-1, 0, -1]]


def _check_covis(store, m, frame_idx, k, include_self, dev, workspace=None):
    from pram_amd import ops
    idx = torch.tensor(frame_idx, dtype=torch.int32, device=dev)
    bf, bc, nf = (x.cpu().numpy() for x in ops.covis_topk(idx, store.tables(dev), k, include_self, workspace))
    assert bf.shape == (len(frame_idx), k)
    ties = 0
    for s, f in enumerate(frame_idx):
        want = TR.get_covisibility_frames(m, store.frame_ids[f], k, include_self=include_self, with_counts=True) if 0 <= f < store.n_frames else []
        ties += len({c for _, c in want}) < len(want)
        n = len(want)
        assert nf[s] == n, (f, k, nf[s], n)
        assert [store.frame_ids[g] for g in bf[s, :n]] == [g for g, _ in want] and bc[s, :n].tolist() == [c for _, c in want], (f, k, include_self)
        assert (bf[s, n:] == -1).all() and (bc[s, n:] == 0).all()
    return ties


def test_covis_topk_exact(scene, dev):
    """Against the restatement: all frames of the scene and of a crafted table with duplicates in the points' frame lists; k 1,
    n_frames - 1 and beyond what exists; both include_self values; a dirty workspace; frames the store does not hold; twice."""
    from pram_amd import ops
    from pram_amd.localization.retrieval import DatabaseStore
    s, m = scene["store"], scene["map"]
    cm = _crafted_map()
    crafted = DatabaseStore(cm["frames"], device=dev, point3D_frame_ids=cm["point3D_frame_ids"])
    assert len(crafted.valid(7)) == 0 and any(len(set(v)) < len(v) for v in cm["point3D_frame_ids"].values())
    ties = 0
    for store, mp in ((s, m), (crafted, cm)):
        F = store.n_frames
        dirty = torch.full((F * F + 7,), 12345, dtype=torch.int32, device=dev)
        for k in (1, 2, F - 1, F + 3):
            for inc in (False, True):
                ties += _check_covis(store, mp, list(range(F)), k, inc, dev)
                ties += _check_covis(store, mp, list(range(F)), k, inc, dev, dirty)
        _check_covis(store, mp, [F - 1, -1, 0, F, 0, 2], 3, False, dev, dirty)
    assert ties > 0
    # the canonical rule on frame 102: 100 before 101
    bf, bc, nf = ops.covis_topk(torch.tensor([2], dtype=torch.int32, device=dev), s.tables(dev), 1, False)
    assert bf.cpu().tolist() == [[0]] and bc.cpu().tolist() == [[40]] and nf.cpu().tolist() == [1]
    # include_self = 1 at the store's own length: the graph the store tabulates on the host, for every reference frame
    vrf = [f for f in range(s.n_frames) if s.is_vrf[f]]
    bf, bc, nf = (x.cpu().numpy() for x in ops.covis_topk(torch.tensor(vrf, dtype=torch.int32, device=dev), s.tables(dev), s.covisibility_frame, True))
    assert len(vrf) == 7
    for i, f in enumerate(vrf):
        a, b = s.covis_off[f], s.covis_off[f + 1]
        assert nf[i] == b - a and np.array_equal(bf[i, :nf[i]], s.covis_frames[a:b]) and np.array_equal(bc[i, :nf[i]], s.covis_count[a:b]), f


def test_covisibility_calls(scene, dev):
    from pram_amd.localization import retrieval as RT
    s, m = scene["store"], scene["map"]
    assert RT.covisibility_pairs(s, COVIS_K, dev) == TR.covisibility_pairs(m, COVIS_K)
    assert RT.covisibility_pairs(s, 50, dev) == TR.covisibility_pairs(m, 50)
    bf, bc, nf = RT.covisible_frames(s, [104, 107], 2, include_self=True, device=dev)
    assert bf.is_cuda and [[s.frame_ids[g] for g in row] for row in bf.cpu().tolist()] == [TR.get_covisibility_frames(m, f, 2, include_self=True) for f in (104, 107)]
    with pytest.raises(ValueError):
        RT.covisible_frames(s, [104, 999], 2, device=dev)
    with pytest.raises(ValueError):
        RT.covisible_frames(s, [104], 0, device=dev)


def _solver(scene, b, n_db, opt_th=None):
    def solve(kpts, xyzs, tag):
        p, th = (b * n_db + tag[1], POSE["threshold"]) if tag[0] == "slot" else (b, opt_th if tag[0] == "refine" else POSE["threshold"])
        return PR.estimate_pose(kpts, xyzs, scene["cams"][b], threshold=th, trials=POSE["trials"], min_inlier_ratio=POSE["min_inlier_ratio"], refine_iters=20, seed=POSE["seed"], p=p)
    return solve


def _same_lists(got, want, keys, what):
    for k in keys:
        g = got[k].cpu().numpy()
        w = np.ascontiguousarray(want[k]).astype(g.dtype)
        assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k, g.shape, w.shape)


def _same_pose(got, ref, what):
    assert got["success"] == ref["success"] and got["num_inliers"] == ref["num_inliers"], (what, got["num_inliers"], ref["num_inliers"])
    if not ref["success"]:
        return 0.0, 0.0
    dq = float(np.abs(got["qvec"] - ref["qvec"]).max())
    dt = float(np.abs(got["tvec"] - ref["tvec"]).max() / (1.0 + np.abs(ref["tvec"]).max()))
    assert dq <= E2E_Q_BAR and dt <= E2E_T_BAR, (what, dq, dt)
    return dq, dt


def _same_result(x, y):
    assert (x is None) == (y is None)
    for k, v in (x or {}).items():
        if k == "slots":
            for sx, sy in zip(v, y[k]):
                _same_result(sx, sy)
        elif k == "refinement":
            _same_result(v, y[k])
        elif torch.is_tensor(v):
            assert torch.equal(v, y[k]), k
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, y[k]), k
        else:
            assert v == y[k], k


def test_hloc(scene, dev):
    """'hloc' on covisible_scene: the stacks equal the restatement's built from the device matcher's matches0 (obs_th fixed to 3
    whatever is passed), the pose equals pose_ref.estimate_pose on them with p = b, query 3 (8 false matches left after the filter,
    refused by the solver: see POSE) takes the first retrieved frame's stored pose, query 4 (an empty list) has none;
    do_covisibility_opt changes nothing; twice, bit-equal.  MI355X, seed 7 (printed, not asserted beyond the equality with the
    restatement): inliers / stacked rows 119 / 130, 147 / 184, 21 / 24 for queries 0 to 2."""
    from pram_amd.localization.retrieval import localize_by_retrieval
    s = scene
    args = (s["features"], TR.SCENE_RETRIEVAL, s["store"], s["net"], s["cams"])
    res = localize_by_retrieval(*args, method="hloc", obs_th=0, **POSE)
    again = localize_by_retrieval(*args, method="hloc", obs_th=7, do_covisibility_opt=True, **POSE)
    for b, r in enumerate(res):
        _same_result(r, again[b])
        db = list(TR.SCENE_RETRIEVAL[b])
        want = TR.pose_estimator_hloc(s["queries"][b], s["map"], db, lambda d, tag: r["slots"][tag[1]]["matches0"].cpu().numpy(), _solver(s, b, 4))
        assert len(r["slots"]) == len(db) and [sl["reference_frame_id"] for sl in r["slots"]] == db
        for j, sl in enumerate(r["slots"]):
            assert int(sl["n_matches"]) == len(want["per_slot"][j]["matched_keypoint_ids"]) and sl["n_ref_kpts"] == len(s["store"].valid(s["store"].index_of[db[j]]))
        assert r["success"] == want["success"] and r["status"] == want["status"] and r["order"] == -1 and r["reference_frame_id"] == want["reference_frame_id"]
        if not want["success"]:
            assert r["num_inliers"] == 0 and r["keypoints_query"].shape == (0, 2) and r["matched_keypoints"].shape[0] == 0
            if db:
                assert np.array_equal(r["qvec"], s["map"]["poses"][db[0]][0]) and np.array_equal(r["tvec"], s["map"]["poses"][db[0]][1])
            else:
                assert r["qvec"] is None and r["tvec"] is None
            continue
        _same_lists(r, want, TR.STACK_KEYS + ("matched_src",), ("hloc", b))
        dq, dt = _same_pose(r, want, ("hloc", b))
        assert np.array_equal(r["inliers"].cpu().numpy(), want["inliers"])
        _same_lists(r, want, ("keypoints_query", "points3D_ids"), ("hloc inliers", b))
        er, ec = PR.pose_errors(PR.qvec_to_rot(r["qvec"]), r["tvec"], s["planted"][b]["R"], s["planted"][b]["t"])
        print(f"retrieval [hloc]: query {b}: {r['num_inliers']}/{r['matched_keypoints'].shape[0]} inliers over {len(db)} frames, dq {dq:.2e} dt {dt:.2e}, "
              f"{er:.4f} deg {ec:.4f} m from the planted camera")
    assert [r["success"] for r in res] == [True, True, True, False, False]
    with pytest.raises(ValueError):
        localize_by_retrieval(s["features"], ([101], [999], [], [], []), s["store"], s["net"], s["cams"], method="hloc", **POSE)
    with pytest.raises(ValueError):
        localize_by_retrieval(*args, method="other", **POSE)


@pytest.mark.parametrize("opt", [False, True], ids=["plain", "covis_opt"])
def test_iterative(scene, dev, opt):
    """'iterative' on covisible_scene, stage by stage against the restatement fed the device matcher's matches0: every slot's
    filtered list and pose (p = query * n_db + slot), the chosen slot and status, with do_covisibility_opt the covisible frames,
    the refinement's stack and pose (p = query, opt_th); query 3 (no row left at obs_th 2) and query 4 (an empty list) fail;
    twice, bit-equal."""
    from pram_amd.localization.retrieval import localize_by_retrieval
    s = scene
    kw = dict(method="iterative", obs_th=2, inlier_th=50, min_best_inliers=10, do_covisibility_opt=opt, covisibility_frame=COVIS_K, opt_th=6.0, **POSE)
    args = (s["features"], TR.SCENE_RETRIEVAL, s["store"], s["net"], s["cams"])
    res = localize_by_retrieval(*args, **kw)
    again = localize_by_retrieval(*args, **kw)
    n_db = 4
    for b, r in enumerate(res):
        _same_result(r, again[b])
        db = list(TR.SCENE_RETRIEVAL[b])

        def matcher(d, tag):
            src = r["slots"] if tag[0] == "slot" else r["refinement"]["slots"]
            return src[tag[1]]["matches0"].cpu().numpy()
        want = TR.pose_estimator_iterative(s["queries"][b], s["map"], db, matcher, _solver(s, b, n_db, 6.0), inlier_th=50, min_best_inliers=10,
                                           do_covisibility_opt=opt, covisibility_frame=COVIS_K, obs_th=2)
        for j, sl in enumerate(r["slots"]):
            assert int(sl["n_matches"]) == len(want["per_slot"][j]["matched_keypoint_ids"]), (b, j)
            _same_pose(sl, want["slot_results"][j], ("slot", b, j))
        assert (r["success"], r["status"], r["best_slot"]) == (want["success"], want["status"], want["best"]), (b, r["status"], want["status"])
        assert r["order"] == want["order"] and r["reference_frame_id"] == want["reference_frame_id"] and r["num_inliers"] == want["num_inliers"], b
        print(f"retrieval [iterative{' + covis' if opt else ''}]: query {b}: status {r['status']} slot {r['order'] - 1} frame {r['reference_frame_id']}, "
              f"{r['num_inliers']} inliers; slots {[(int(sl['n_matches']), sl['num_inliers']) for sl in r['slots']]}")
        if not want["success"]:
            assert r["keypoints_query"].shape == (0, 2) and r["num_inliers"] == (-1 if db else 0) and r.get("refinement") is None
            assert (r["qvec"] is None) == (not db) and (not db or np.array_equal(r["tvec"], s["map"]["poses"][db[0]][1]))
            continue
        _same_lists(r, want, TR.STACK_KEYS, ("kept", b))
        assert np.array_equal(r["inliers"].cpu().numpy(), want["inliers"])
        _same_lists(r, want, ("keypoints_query", "points3D_ids"), ("inliers", b))
        if opt:
            x, wx = r["refinement"], want["refinement"]
            assert x["covisible_frame_ids"] == wx["covisible_frame_ids"] and len(x["slots"]) == len(wx["per_slot"])
            _same_lists(x, wx, TR.STACK_KEYS + ("matched_src",), ("refinement", b))
            _same_pose(x, wx, ("refinement", b))
            assert np.array_equal(x["inliers"].cpu().numpy(), wx["inliers"])
            assert np.array_equal(r["qvec"], x["qvec"]) and np.array_equal(r["tvec"], x["tvec"])
        dq = float(np.abs(r["qvec"] - want["qvec"]).max())
        assert dq <= E2E_Q_BAR, (b, dq)
        er, ec = PR.pose_errors(PR.qvec_to_rot(r["qvec"]), r["tvec"], s["planted"][b]["R"], s["planted"][b]["t"])
        print(f"retrieval [iterative{' + covis' if opt else ''}]: query {b}: {er:.4f} deg {ec:.4f} m from the planted camera")
    assert [r["success"] for r in res[3:]] == [False, False] and res[0]["success"] and res[1]["success"]


def test_adagml_grouped_path(scene, dev):
    from pram_amd.nets.adagml import AdaGML
    from pram_amd.localization.retrieval import localize_by_retrieval
    net = AdaGML({})
    net.load_state_dict(H.adagml_sd(), strict=True)
    net = net.to(dev).eval()
    s = scene
    res = localize_by_retrieval(s["features"], TR.SCENE_RETRIEVAL, s["store"], net, s["cams"], method="hloc", **POSE)
    for b, r in enumerate(res):
        want = TR.pose_estimator_hloc(s["queries"][b], s["map"], list(TR.SCENE_RETRIEVAL[b]), lambda d, tag: r["slots"][tag[1]]["matches0"].cpu().numpy(),
                                      lambda k, x, tag: {"success": False})
        assert int(sum(int(sl["n_matches"]) for sl in r["slots"])) == len(want["matched_keypoint_ids"]), b
        if r["success"]:
            _same_lists(r, want, TR.STACK_KEYS, ("adagml", b))
    print("retrieval [adagml]:", [(r["success"], r["num_inliers"]) for r in res])
    assert sum(int(sl["n_matches"]) for r in res for sl in r["slots"]) > 50


def test_ctypes_entries(hip_lib, dev):
    """The four entries through ctypes alone on hand-written tables, each with a null pointer and a bad size."""
    L = hip_lib
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E_ARG = -1
    # three frames of 4, 2, 3 rows; valid rows: frame 0 -> rows 1, 3; frame 1 -> none; frame 2 -> 6, 7, 8
    frame_off, valid_off, valid_rows = i32([0, 4, 6, 9, 0]), i32([0, 2, 2, 5, 0]), i32([1, 3, 6, 7, 8, 0])
    retrieval, counts = i32([[2, 1], [0, 3]]), i32([5, 6])
    plan = torch.full((10, 4), -9, dtype=torch.int32, device=dev)

    def run_plan(n_db=2, ret=retrieval, n_frames=3, enable=None):
        return L.pram_retr_plan(p(ret), p(counts), p(enable), p(frame_off), p(valid_off), 2, n_db, n_frames, 5, p(plan), st)
    assert run_plan() == 0
    assert plan.cpu().tolist() == [[0, 0, 1, 1], [-1] * 4, [2, -1, 0, -1], [0] * 4, [5, 0, 6, 0], [3, 0, 2, 0], [-1] * 4, [6, 0, 0, 0], [2, -1, 0, -1], [0, 1, 0, 1]]
    assert run_plan(enable=i32([0, 1])) == 0 and plan[2].tolist() == [-1, -1, 0, -1]
    assert run_plan(n_db=0) == E_ARG and b"n_db" in L.pram_last_error()
    assert run_plan(ret=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_plan(n_frames=-1) == E_ARG
    # filter: points 11 (3 observations), 12 (1), 15 (2); two pairs of t0 = 4
    pt_ids, pt_off = i64([11, 12, 15]), i32([0, 3, 4, 6, 0])
    mk = lambda base: {"ids": i64(np.arange(8).reshape(2, 4) + base), "kp": torch.arange(16, dtype=torch.float32, device=dev).reshape(2, 4, 2) + base,
                       "rk": torch.arange(16, dtype=torch.float32, device=dev).reshape(2, 4, 2) - base, "p3": i64([[11, 12, 15, 99], [15, 11, 11, 12]]),
                       "xyz": torch.arange(24, dtype=torch.float64, device=dev).reshape(2, 4, 3) / 7 + base, "sid": i32(np.arange(8).reshape(2, 4) % 5)}
    r, o = mk(100), mk(-50)
    r_count, m_count = i32([4, 3]), i32([-5, -5])
    order = ("ids", "kp", "rk", "p3", "xyz", "sid")

    def run_filter(obs_th=2, t0=4, first=r["ids"], xyz_out=o["xyz"], out_first=o["ids"]):
        return L.pram_retr_filter(p(first), *[p(r[k]) for k in order[1:]], p(r_count), 2, t0, p(pt_ids), p(pt_off), 3, obs_th, p(out_first),
                                  *[p(o[k]) for k in order[1:4]], C.c_void_p(xyz_out.data_ptr()), p(o["sid"]), p(m_count), st)
    assert run_filter() == 0
    assert m_count.tolist() == [2, 3] and o["ids"][0, :2].tolist() == [100, 102] and o["ids"][1, :3].tolist() == [104, 105, 106] and o["ids"][0, 2:].tolist() == [-48, -47]
    assert torch.equal(o["xyz"][0, :2], r["xyz"][0, [0, 2]]) and torch.equal(o["kp"][1, :3], r["kp"][1, :3]) and o["p3"][0, :2].tolist() == [11, 15]
    assert run_filter(obs_th=0) == 0 and m_count.tolist() == [4, 3]
    assert run_filter(t0=-1) == E_ARG and b"t0" in L.pram_last_error()
    assert run_filter(first=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_filter(xyz_out=o["xyz"].view(torch.float32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
    assert run_filter(out_first=r["ids"]) == E_ARG and b"must not be the input" in L.pram_last_error()
    # select
    succ, inl, cnt, chosen = i32([1, 1, 1, 0]), i32([20, 60, 9, 99]), i32([9, 9, 9, 9]), i32([[-9] * 3] * 2)

    def run_select(n_db=2, s_=succ):
        return L.pram_retr_select(p(s_), p(inl), p(cnt), 2, n_db, 50, 10, p(chosen), st)
    assert run_select() == 0 and chosen.tolist() == [[1, 1, 1], [-1, 0, 0]]
    assert run_select(n_db=0) == E_ARG and b"n_db" in L.pram_last_error()
    assert run_select(s_=None) == E_ARG and b"null" in L.pram_last_error()
    # covisibility: rows' point ids; points 11 -> frames [0, 2, 2], 12 -> [1], 15 -> [2, 0]
    point3d_ids, pt_frames = i64([-1, 11, -1, 15, -1, -1, 11, 12, 15]), i32([0, 2, 2, 1, 2, 0, 0])
    frames, hist = i32([0, 2, 1]), i32(np.full((3, 3), 77))
    bf, bc, nf = i32(np.full((3, 2), -9)), i32(np.full((3, 2), -9)), i32([-9] * 3)

    def run_covis(k=2, n_frames=3, include_self=0, hist_=hist, ids=point3d_ids):
        return L.pram_covis_topk(p(frames), 3, p(valid_off), p(valid_rows), C.c_void_p(ids.data_ptr()), 9, 5, p(pt_ids), p(pt_off), p(pt_frames), 3, 6, n_frames, k,
                                 include_self, p(hist_), p(bf), p(bc), p(nf), st)
    assert run_covis() == 0      # frame 0 sees 11 and 15: frame 2 three times; frame 2 sees 11, 12, 15: frame 0 twice, frame 1 once
    assert hist.tolist() == [[0, 0, 3], [2, 1, 0], [0, 0, 0]] and bf.tolist() == [[2, -1], [0, 1], [-1, -1]] and bc.tolist() == [[3, 0], [2, 1], [0, 0]] and nf.tolist() == [1, 2, 0]
    assert run_covis(include_self=1) == 0 and hist.tolist() == [[2, 0, 3], [2, 1, 3], [0, 0, 0]] and bf.tolist() == [[2, 0], [2, 0], [-1, -1]]
    torch.cuda.synchronize()
    assert run_covis(k=0) == E_ARG and b"k >= 1" in L.pram_last_error()
    assert run_covis(n_frames=0) == E_ARG
    assert run_covis(hist_=None) == E_ARG and b"null" in L.pram_last_error()
    assert run_covis(ids=point3d_ids.view(torch.int32).view(-1)[1:]) == E_ARG and b"8-byte" in L.pram_last_error()
