"""GPU: image retrieval (pram_amd.localization.image_retrieval, csrc/imgret.hip) against the numpy restatement
tests/imgret_ref.py: every kernel on its own (bit-equal where the restatement has the kernel's order of operations, exact on
integer data, within the derived bound of an fp32 chain on real vectors), the refusals, the C entries through ctypes, and the stage
end to end on two planted scenes: into localize_by_retrieval and into mapper.reconstruct.  tests/test_imgret_cpu.py holds the
margins of the discrete assertions made here."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import helpers as H
from tests import imgret_ref as IR
from tests import mapper_ref as MR
from tests import pose_ref as PR
from tests import retrieval_ref as TR

pytestmark = pytest.mark.gpu

E_ARG = -1
ROT_FACTOR, CENTRE_FACTOR, POINT_SHARE = 2.0, 2.0, 0.9      # the bars of tests/test_gpu_mapper.py::test_planted_scene_accuracy
E2E_Q_BAR, E2E_T_BAR = 1e-8, 2e-8                           # and of tests/test_gpu_retrieval.py for the poses of 'hloc'
POSE = dict(threshold=4.0, trials=300, seed=4, min_inlier_ratio=0.6)      # tests/test_gpu_retrieval.py's


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    from pram_amd.localization import image_retrieval
    return image_retrieval


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view(np.uint8)


def _same_bits(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = np.ascontiguousarray(want).astype(got.dtype)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), what


# ---------------------------------------------------------------- 1. assign
@pytest.mark.parametrize("k", IR.ASSIGN_K)
def test_assign_exact(dev, k):
    """Labels exact (the planted duplicate centres: ties to the lower index), dist bit-equal, at every n_rows."""
    from pram_amd import ops
    for n in IR.ASSIGN_ROWS:
        x, c = IR.assign_case(n, k)
        lab, dist = ops.imgret_assign(_up(x, dev), _up(c, dev))
        want_lab, want_dist = IR.assign(x, c)
        assert np.array_equal(lab.cpu().numpy(), want_lab), (n, k)
        _same_bits(dist, want_dist, ("dist", n, k))
        if k >= 2:
            assert (want_lab != k - 1).all()


# ---------------------------------------------------------------- 2. aggregate and normalise
def test_aggregate_normalize_exact(dev, M):
    """The flat layout (images of 0, 1, 65 and 300 rows) and the padded layout with NaN behind every count: sums, n_assigned and the
    float32 vectors bit-equal to the restatement, whatever the image_chunk."""
    from pram_amd import ops
    c, (x, first, cnt), batch, counts = IR.aggregate_case()
    dc, dx = _up(c, dev), _up(x, dev)
    lab, _ = ops.imgret_assign(dx, dc)
    want_lab, _ = IR.assign(x, c)
    assert np.array_equal(lab.cpu().numpy(), want_lab)
    sums, n = ops.imgret_aggregate(dx, lab, dc, _up(first.astype(np.int32), dev), _up(cnt.astype(np.int32), dev))
    want_sums, want_n = IR.aggregate(x, want_lab, c, first, cnt)
    _same_bits(sums, want_sums, "sums")
    assert np.array_equal(n.cpu().numpy(), want_n) and not want_n[0].any() and (want_n[1] == 0).sum() == IR.AGG_K - 1
    want_out = IR.normalize(want_sums)
    _same_bits(ops.imgret_normalize(sums), want_out, "out")
    assert not want_out[0].any()
    vocab = M.Vocabulary(dc)
    off = np.concatenate([first, [int(cnt.sum())]])
    frames = [{"descriptors": x[a:b]} for a, b in zip(off[:-1], off[1:])]
    for chunk in (1, 3, 1024):
        _same_bits(M.global_descriptors(vocab, frames, image_chunk=chunk), want_out, ("flat", chunk))
    # the padded layout: first = b * N, the rows behind a count are NaN and never reach a sum
    db = _up(batch, dev)
    plab, _ = ops.imgret_assign(db.view(-1, IR.DIM), dc)
    pfirst = _up((np.arange(len(counts)) * IR.PADDED_N).astype(np.int32), dev)
    psums, pn = ops.imgret_aggregate(db.view(-1, IR.DIM), plab, dc, pfirst, _up(counts.astype(np.int32), dev))
    ws, wn, wout = IR.padded_vlad(batch, counts, c)
    _same_bits(psums, ws, "padded sums")
    assert np.array_equal(pn.cpu().numpy(), wn)
    feats = {"descriptors": db, "counts": _up(counts.astype(np.int32), dev)}
    for chunk in (1, 3, 1024):
        got = M.global_descriptors(vocab, feats, image_chunk=chunk)
        assert torch.isfinite(got).all()
        _same_bits(got, wout, ("padded", chunk))


# ---------------------------------------------------------------- 3. vocabulary
def test_vocabulary_exact(dev, M, tmp_path):
    """n = 1025, k = 16: the centres after 1 and after 3 iterations bit-equal to the restatement and on a repeat; the centre that
    starts as a copy of a lower one gets no row in the first iteration and keeps its value."""
    x, picks = IR.vocab_case()
    assert np.array_equal(M.initial_rows(IR.VOCAB_N, IR.VOCAB_K, IR.VOCAB_SEED), picks)
    one = M.train_vocabulary(x, k=IR.VOCAB_K, iters=1, seed=IR.VOCAB_SEED, device=dev)
    _same_bits(one.centres, IR.train_vocabulary(x, IR.VOCAB_K, 1, IR.VOCAB_SEED), "one iteration")
    _same_bits(one.centres[IR.VOCAB_STARVED], x[picks[IR.VOCAB_STARVED]], "the starved centre")
    v = M.train_vocabulary(_up(x, dev), k=IR.VOCAB_K, iters=IR.VOCAB_ITERS, seed=IR.VOCAB_SEED, device=dev)
    _same_bits(v.centres, IR.train_vocabulary(x, IR.VOCAB_K, IR.VOCAB_ITERS, IR.VOCAB_SEED), "three iterations")
    again = M.train_vocabulary(x, k=IR.VOCAB_K, iters=IR.VOCAB_ITERS, seed=IR.VOCAB_SEED, device=dev)
    assert torch.equal(v.centres, again.centres) and v.centres.dtype == torch.float32 and v.k == IR.VOCAB_K
    v.save(tmp_path / "vocab.npz")
    back = M.Vocabulary.load(tmp_path / "vocab.npz", device=dev)
    assert torch.equal(back.centres, v.centres) and back.centres.is_cuda


# ---------------------------------------------------------------- 4. top-k with exact arithmetic
@pytest.mark.parametrize("nq,nd,L,k", IR.TOPK_CASES)
def test_topk_integer_exact(dev, nq, nd, L, k):
    """Entries from {-1, 0, 1}: idx and sim equal the integer restatement exactly, order included, with and without exclude = self,
    the same bits for splits 1, 3 and 8; a db_valid that leaves nothing gives -1 / 0 everywhere."""
    from pram_amd import ops
    q, db = IR.topk_int_case(nq, nd, L)
    S = q.astype(np.float64) @ db.astype(np.float64).T + 0.0      # + 0.0: no -0.0
    dq, ddb = _up(q, dev), _up(db, dev)
    excl = IR.self_exclude(nq, nd)
    valid = (np.arange(nd) % 3 != 1).astype(np.uint8)
    for e, v in ((None, None), (excl, None), (excl, valid)):
        want_idx, want_sim = IR.topk(S, k, exclude=e, db_valid=v)
        for splits in IR.TOPK_SPLITS:
            idx, sim = ops.imgret_topk(dq, ddb, k, None if e is None else _up(e, dev), None if v is None else _up(v, dev), splits)
            assert np.array_equal(idx.cpu().numpy(), want_idx), (splits, e is None, v is None)
            _same_bits(sim, want_sim.astype(np.float32), ("sim", splits))
    if k > nd:
        assert (want_idx[:, nd:] == -1).all()
    idx, sim = ops.imgret_topk(dq, ddb, k, None, torch.zeros(nd, dtype=torch.uint8, device=dev), 3)
    assert (idx == -1).all() and not sim.any()


# ---------------------------------------------------------------- 5. top-k on real vectors
@pytest.fixture(scope="module")
def covis(dev, M):
    c = IR.covisible()
    x = c["rows"]
    vocab = M.train_vocabulary(x, k=IR.COVIS_K, iters=IR.COVIS_ITERS, seed=IR.COVIS_SEED, device=dev)
    from pram_amd.localization.retrieval import DatabaseStore
    poses = {f["id"]: (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)) for f in c["map"]["frames"]}
    m = dict(c["map"], poses=poses)
    store = DatabaseStore(m["frames"], m["seg_ref_frame_ids"], 0, device=dev, covisibility_frame=4, poses=poses)
    feats, _ = CR.batch_features(c["queries"], dev)
    return dict(c, map=m, vocab=vocab, store=store, features=feats, index=M.RetrievalIndex(store, vocab))


def _check_real(q, db, k, idx, sim, exclude=None):
    """The checks of the issue's part 5 -> the largest |sim - float64 product| seen."""
    L = q.shape[1]
    eps = IR.topk_eps(L)
    S = q.astype(np.float64) @ db.astype(np.float64).T
    worst = 0.0
    for i in range(len(q)):
        got = [(int(j), float(s)) for j, s in zip(idx[i], sim[i]) if j >= 0]
        allowed = [j for j in range(len(db)) if exclude is None or exclude[i] != j]
        assert len(got) == min(k, len(allowed)) and len({j for j, _ in got}) == len(got) and all(j in allowed for j, _ in got)
        for j, s in got:
            worst = max(worst, abs(s - S[i, j]))
            assert abs(s - S[i, j]) <= eps, (i, j, s, S[i, j])
        for (j0, s0), (j1, s1) in zip(got[:-1], got[1:]):
            assert s0 > s1 or (s0 == s1 and j0 < j1), (i, j0, j1)
        if got:
            low = min(S[i, j] for j, _ in got)
            assert all(S[i, j] <= low + 2 * eps for j in allowed if j not in {g for g, _ in got}), i
    return worst


def test_topk_real_vectors(dev, M, covis):
    """Unit VLAD vectors of both scenes (L = 2048 at k = 16, L = 8192 at k = 64) against the float64 product of the same fp32
    inputs within eps = 2 L 2^-24.  MI355X: the figures are in profiles/imgret_parity.md."""
    vf = M.global_descriptors(covis["vocab"], covis["map"]["frames"])
    vq = M.global_descriptors(covis["vocab"], covis["features"])
    _same_bits(vf, covis["v_frames"], "the frames' vectors")
    _same_bits(vq, covis["v_queries"], "the queries' vectors")
    _same_bits(covis["index"].descriptors, covis["v_frames"], "the store's vectors")
    both = torch.cat([vf, vq])
    idx, sim = M.retrieve(both, vf, 5)
    w1 = _check_real(both.cpu().numpy(), vf.cpu().numpy(), 5, idx.cpu().numpy(), sim.cpu().numpy())
    st = IR.street()
    x, _, _ = IR.flat(st["frames"])
    v64 = M.train_vocabulary(x, k=64, iters=5, seed=1, device=dev)
    g = M.global_descriptors(v64, st["frames"])
    assert g.shape == (IR.STREET_FRAMES, 64 * IR.DIM)
    n = len(g)
    ex = np.arange(n, dtype=np.int32)
    w2 = 0.0
    for splits in (None, 1, 2):
        idx, sim = M.retrieve(g, g, 6, exclude=ex, splits=splits)
        w2 = max(w2, _check_real(g.cpu().numpy(), g.cpu().numpy(), 6, idx.cpu().numpy(), sim.cpu().numpy(), exclude=ex))
    print(f"imgret parity: largest |sim - fp64| {w1:.3e} at L = 2048 (bound {IR.topk_eps(2048):.3e}), {w2:.3e} at L = 8192 (bound {IR.topk_eps(8192):.3e})")
    # a length that is no multiple of 128 is zero-padded: NetVLAD-like vectors from outside
    rng = np.random.RandomState(8)
    a = rng.standard_normal((5, 200)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    idx, sim = M.retrieve(a, _up(a, dev), 2)
    assert idx[:, 0].tolist() == list(range(5)) and (np.abs(sim[:, 0].cpu().numpy() - 1.0) < IR.topk_eps(256)).all()


# ---------------------------------------------------------------- 6. refusals, 9. the C entries through ctypes
def test_ctypes_entries_and_refusals(hip_lib, dev):
    """Every entry through ctypes alone on small tables, then the refusals: PRAM_E_ARG with the entry's name in pram_last_error."""
    L = hip_lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, c = IR.assign_case(65, 16)
    dx, dc = _up(x, dev), _up(c, dev)
    lab = torch.full((65,), -9, dtype=torch.int32, device=dev)
    dist = torch.zeros(65, dtype=torch.float64, device=dev)
    assert L.pram_imgret_assign(p(dx), 65, p(dc), 16, p(lab), p(dist), st) == 0
    want_lab, want_dist = IR.assign(x, c)
    assert np.array_equal(lab.cpu().numpy(), want_lab)
    _same_bits(dist, want_dist, "dist")
    first, count = torch.tensor([0, 40, 40], dtype=torch.int32, device=dev), torch.tensor([40, 0, 25], dtype=torch.int32, device=dev)
    sums = torch.full((3, 16, 128), 7.0, dtype=torch.float64, device=dev)
    n_as = torch.full((3, 16), -9, dtype=torch.int32, device=dev)
    assert L.pram_imgret_aggregate(p(dx), p(lab), 65, p(dc), 16, p(first), p(count), 3, p(sums), p(n_as), st) == 0
    want_sums, want_n = IR.aggregate(x, want_lab, c, [0, 40, 40], [40, 0, 25])
    _same_bits(sums, want_sums, "sums")
    assert np.array_equal(n_as.cpu().numpy(), want_n)
    out = torch.full((3, 16 * 128), 9.0, dtype=torch.float32, device=dev)
    assert L.pram_imgret_normalize(p(sums), 3, 16, p(out), st) == 0
    _same_bits(out, IR.normalize(want_sums), "out")
    total, total_n = torch.zeros(16, 128, dtype=torch.float64, device=dev), torch.zeros(16, dtype=torch.int32, device=dev)
    assert L.pram_imgret_fold(p(sums), p(n_as), 3, 16, p(total), p(total_n), st) == 0
    _same_bits(total, (want_sums[0] + want_sums[1]) + want_sums[2], "total")
    assert np.array_equal(total_n.cpu().numpy(), want_n.sum(0))
    cen = dc.clone()
    assert L.pram_imgret_update(p(cen), p(total), p(total_n), 16, st) == 0
    tot, cnt = total.cpu().numpy(), want_n.sum(0)
    want_c = c.copy()
    want_c[cnt > 0] = (c[cnt > 0].astype(np.float64) + tot[cnt > 0] / cnt[cnt > 0, None]).astype(np.float32)
    _same_bits(cen, want_c, "centres")
    q, db = IR.topk_int_case(5, 200, 256)
    dq, ddb = _up(q, dev), _up(db, dev)
    need = L.pram_imgret_topk_workspace_bytes(5, 7, 2)
    assert need == 5 * 2 * 7 * 8
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    idx, sim = torch.full((5, 7), -9, dtype=torch.int32, device=dev), torch.full((5, 7), -9.0, dtype=torch.float32, device=dev)

    def topk(q_=dq, nd=200, Ln=256, k=7, splits=2, ws_=ws, ws_bytes=need, idx_=idx):
        return L.pram_imgret_topk(p(q_), 5, p(ddb), nd, Ln, None, None, k, splits, p(ws_), ws_bytes, p(idx_), p(sim), st)
    assert topk() == 0
    want_idx, want_sim = IR.topk(q.astype(np.float64) @ db.astype(np.float64).T, 7)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(sim.cpu().numpy(), want_sim.astype(np.float32))
    # refusals: nothing is launched, the outputs keep their bits
    idx.fill_(-9)
    for kw, word in ((dict(k=0), b"k"), (dict(k=65), b"k"), (dict(Ln=200), b"multiple"), (dict(Ln=0), b"multiple"), (dict(nd=0), b"nd"),
                     (dict(q_=None), b"null"), (dict(ws_=None), b"null"), (dict(idx_=None), b"null"), (dict(ws_bytes=need - 1), b"workspace"),
                     (dict(splits=0), b"splits"), (dict(splits=1025), b"splits"), (dict(q_=dq.view(-1)[1:]), b"misaligned")):
        assert topk(**kw) == E_ARG, kw
        msg = L.pram_last_error()
        assert b"pram_imgret_topk" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (idx == -9).all()
    assert L.pram_imgret_assign(p(dx), 65, p(dc), 0, p(lab), p(dist), st) == E_ARG and b"pram_imgret_assign" in L.pram_last_error()
    assert L.pram_imgret_assign(p(dx), 65, p(dc), 257, p(lab), p(dist), st) == E_ARG and b"256" in L.pram_last_error()
    assert L.pram_imgret_assign(None, 65, p(dc), 16, p(lab), p(dist), st) == E_ARG and b"null" in L.pram_last_error()
    assert L.pram_imgret_assign(p(dx), -1, p(dc), 16, p(lab), p(dist), st) == E_ARG
    assert L.pram_imgret_assign(p(dx), 65, p(dc), 16, p(lab), C.c_void_p(dist.data_ptr() + 4), st) == E_ARG and b"misaligned" in L.pram_last_error()
    assert L.pram_imgret_aggregate(p(dx), p(lab), 65, p(dc), 300, p(first), p(count), 3, p(sums), p(n_as), st) == E_ARG and b"pram_imgret_aggregate" in L.pram_last_error()
    assert L.pram_imgret_aggregate(p(dx), None, 65, p(dc), 16, p(first), p(count), 3, p(sums), p(n_as), st) == E_ARG and b"null" in L.pram_last_error()
    assert L.pram_imgret_aggregate(p(dx), p(lab), 65, p(dc), 16, p(first), p(count), -1, p(sums), p(n_as), st) == E_ARG
    assert L.pram_imgret_normalize(p(sums), 3, 0, p(out), st) == E_ARG and b"pram_imgret_normalize" in L.pram_last_error()
    assert L.pram_imgret_normalize(None, 3, 16, p(out), st) == E_ARG and b"null" in L.pram_last_error()
    assert L.pram_imgret_fold(p(sums), p(n_as), -1, 16, p(total), p(total_n), st) == E_ARG and b"pram_imgret_fold" in L.pram_last_error()
    assert L.pram_imgret_update(None, p(total), p(total_n), 16, st) == E_ARG and b"pram_imgret_update" in L.pram_last_error()
    # the Python side hands the refusal on
    from pram_amd import ops
    from pram_amd._lib import PramHipError
    with pytest.raises(PramHipError):
        ops.imgret_topk(dq, ddb, 65)
    with pytest.raises(PramHipError):
        ops.imgret_topk(dq[:, :200].contiguous(), ddb[:, :200].contiguous(), 3)


# ---------------------------------------------------------------- 7. the planted covisible scene
def test_covisible_scene(dev, M, covis):
    """refine_ref.covisible_scene: every frame's first retrieved frame is the one it shares most point ids with (frame 2: 0 or 1), the
    first two of queries 0 to 2 are the two frames that share most pool points with their windows, the 10-keypoint query finds frame
    7, the empty query gets an empty list; RetrievalIndex.query's lists then go into localize_by_retrieval(method='hloc') and
    queries 0 to 2 meet what tests/test_gpu_retrieval.py::test_hloc asserts of its hand-written lists."""
    from pram_amd.localization.retrieval import localize_by_retrieval
    c, index, store = covis, covis["index"], covis["store"]
    share = c["share"]
    F = len(share)
    pairs_idx, _ = M.retrieve(index.descriptors, index.descriptors, 3, exclude=np.arange(F, dtype=np.int32))
    pairs_idx = pairs_idx.cpu().numpy()
    for f in range(F):
        assert share[f, pairs_idx[f, 0]] == share[f].max(), (f, pairs_idx[f].tolist(), share[f].tolist())
    lists = index.query(c["features"], 3)
    ids = [fr["id"] for fr in c["map"]["frames"]]
    pos = {fid: i for i, fid in enumerate(ids)}
    print(f"imgret: covisible scene lists {lists}")
    for b, want in enumerate(IR.COVIS_QUERY_TOP2):
        assert {pos[fid] for fid in lists[b][:2]} == set(want), (b, lists[b])
    assert pos[lists[3][0]] == 7 and lists[4] == [] and [len(l) for l in lists[:4]] == [3, 3, 3, 3]
    # the restatement's lists, cut with the margins tests/test_imgret_cpu.py holds
    want_idx, _ = IR.topk(c["v_queries"].astype(np.float64) @ c["v_frames"].astype(np.float64).T, 3)
    assert [[pos[fid] for fid in l] for l in lists[:4]] == want_idx[:4].tolist()
    # into the localizer: test_hloc's assertions for queries 0 to 2, with these lists in place of SCENE_RETRIEVAL
    from pram_amd.nets.gml import GML
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    net = net.to(dev).eval()
    cams = [p["cam"] for p in c["planted"]]
    res = localize_by_retrieval(c["features"], lists, store, net, cams, method="hloc", **POSE)
    real = lambda q: {k: (v[:q["count"]] if isinstance(v, np.ndarray) else v) for k, v in q.items() if k != "padded"}
    for b in range(3):
        r, db = res[b], list(lists[b])

        def solve(kpts, xyzs, tag, b=b):
            return PR.estimate_pose(kpts, xyzs, cams[b], threshold=POSE["threshold"], trials=POSE["trials"], min_inlier_ratio=POSE["min_inlier_ratio"],
                                    refine_iters=20, seed=POSE["seed"], p=b)
        want = TR.pose_estimator_hloc(real(c["queries"][b]), c["map"], db, lambda d, tag: r["slots"][tag[1]]["matches0"].cpu().numpy(), solve)
        assert len(r["slots"]) == len(db) and [sl["reference_frame_id"] for sl in r["slots"]] == db
        assert r["success"] and want["success"] and r["status"] == want["status"] and r["num_inliers"] == want["num_inliers"]
        dq = float(np.abs(r["qvec"] - want["qvec"]).max())
        dt = float(np.abs(r["tvec"] - want["tvec"]).max() / (1.0 + np.abs(want["tvec"]).max()))
        assert dq <= E2E_Q_BAR and dt <= E2E_T_BAR, (b, dq, dt)
        assert np.array_equal(r["inliers"].cpu().numpy(), want["inliers"])
        er, ec = PR.pose_errors(PR.qvec_to_rot(r["qvec"]), r["tvec"], c["planted"][b]["R"], c["planted"][b]["t"])
        print(f"imgret -> hloc: query {b}: {r['num_inliers']}/{r['matched_keypoints'].shape[0]} inliers over {db}, {er:.4f} deg {ec:.4f} m from the planted camera")
    assert not res[3]["success"] or res[3]["reference_frame_id"] in lists[3]
    assert not res[4]["success"] and res[4]["qvec"] is None


# ---------------------------------------------------------------- 8. through the mapper
def test_street_scene_through_the_mapper(dev, M):
    """The street scene: pairs_from_retrieval(num_matched = 4) on the device's vectors equals the restatement's list, every listed
    pair shares at least STREET_MIN_SHARE planted points, and mapper.reconstruct on these pairs registers every frame it registers
    on the planted neighbour list (frames at most three apart) within test_planted_scene_accuracy's bars against that run: the
    largest rotation and centre error at most twice, the points at least 0.9.  MI355X: both rows are in profiles/imgret_parity.md."""
    from pram_amd.localization import mapper as MP
    st = IR.street()
    s, frames = st["scene"], st["frames"]
    x, _, _ = IR.flat(frames)
    vocab = M.train_vocabulary(x, k=IR.STREET_K, iters=IR.STREET_ITERS, seed=IR.STREET_SEED, device=dev)
    _same_bits(vocab.centres, st["centres"], "the vocabulary")
    g = M.global_descriptors(vocab, frames)
    _same_bits(g, st["vectors"], "the vectors")
    pairs = M.pairs_from_retrieval(g, IR.STREET_MATCHED)
    assert pairs == st["pairs"]
    assert len({frozenset(p) for p in pairs}) == len(pairs) and all(a != b for a, b in pairs)
    assert min(s["share"][a, b] for a, b in pairs) >= IR.STREET_MIN_SHARE
    runs = {}
    for name, pr in (("retrieval", pairs), ("neighbours", s["neighbour_pairs"])):
        runs[name] = MP.reconstruct(s["frames"], s["cameras"], np.array(pr, dtype=np.int64), IR.street_matches(s, pr), dev)
        assert runs[name]["report"]["success"], (name, runs[name]["report"])
    reg_n, reg_r = runs["neighbours"]["registered"], runs["retrieval"]["registered"]
    assert reg_n.sum() >= 3 and (reg_r | ~reg_n).all(), (reg_n.tolist(), reg_r.tolist())
    reg = np.nonzero(reg_n & reg_r)[0]
    true_c = s["table"][:, 12:15]
    fig = {}
    for name, r in runs.items():
        sRt = MP.similarity_from_centres(MR.centres_of(r["qvecs"], r["tvecs"])[reg], true_c[reg])
        rot, cen = MR.pose_errors(r["qvecs"], r["tvecs"], s, reg, sRt)
        fig[name] = (rot, cen, len(r["point_ids"]))
        print(f"imgret -> mapper [{name}]: {len(pairs) if name == 'retrieval' else len(s['neighbour_pairs'])} pairs, "
              f"registered {int(r['registered'].sum())}, largest rotation error {rot:.5f} deg, largest centre error {cen:.6f}, points {len(r['point_ids'])}")
    a, b = fig["retrieval"], fig["neighbours"]
    print(f"imgret -> mapper ratios: rotation {a[0] / b[0]:.3f}, centre {a[1] / b[1]:.3f}, points {a[2] / b[2]:.3f}")
    assert a[0] <= ROT_FACTOR * b[0] and a[1] <= CENTRE_FACTOR * b[1] and a[2] >= POINT_SHARE * b[2], fig
