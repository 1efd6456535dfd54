"""GPU: the three kernels at the front of the pipeline — pram_score_map_f32, pram_simple_nms_f32, pram_select_keypoints_f32
(pram_amd/csrc/sfd2_post.hip) — swept over every class of shape and content that steers a branch of theirs, against the plain
references of oracle/ref_cpu.py; plus the empty extents of these entries and the bounds of pram_score_lookup_f32.

The cases and the reasons for them are in tests/detector_cases.py; tests/test_detector_cases_cpu.py shows, without a GPU, that
each case reaches the branch it names.  Everything that is an index, a count or a copied score must be equal bit for bit.  The
score map is held to a bar on its relative error that is derived from the arithmetic, not measured (detector_cases.score_bar),
on every element."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import detector_cases as D

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
SEL = D.sel_cases()


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ score map
@pytest.mark.parametrize("regime", list(D.SCORE_REGIMES))
def test_score_map_every_element_under_the_derived_bar(dev, regime):
    from pram_amd import ops
    worst = 0.0
    for shape in D.SCORE_SHAPES:
        lg = D.score_logits(shape, regime)
        out = ops.score_map(lg.permute(0, 2, 3, 1).contiguous().to(dev))
        ratio, _ = D.score_ratio(out, lg)
        worst = max(worst, ratio)
        if regime == "equal":
            assert bool((out.cpu() == np.float32(1.0) / np.float32(65.0)).all()), shape
    print(f"score map {regime}: largest error / bar = {worst:.3f}  (bar = (|x - mx| + {D.SCORE_CONST:g}) * 2^-24 relative)")
    assert worst <= 1.0, (regime, worst)


def test_score_map_writes_its_own_cells_only(dev, hip_lib):
    """the cell guard at every remainder: the entry on a sentinel-filled buffer longer than the map leaves the tail alone"""
    from pram_amd import ops
    for shape in D.SCORE_SHAPES:
        B, hc, wc = shape
        lg = D.score_logits(shape, "normal").permute(0, 2, 3, 1).contiguous().to(dev)
        n = B * hc * wc * 64
        buf = torch.full((n + 4 * 64,), SENTINEL, device=dev)
        assert hip_lib.pram_score_map_f32(lg.data_ptr(), buf.data_ptr(), B, hc, wc, _st()) == 0
        assert torch.equal(buf[:n].view(B, hc * 8, wc * 8), ops.score_map(lg)) and bool((buf[n:] == SENTINEL).all()), shape


# ------------------------------------------------------------------------------------------------ simple_nms
def _nms_entry(hip_lib, s, radius, fill):
    """the C entry with a caller-owned workspace prefilled with the byte ``fill``, on an output prefilled with the sentinel"""
    B, h, w = s.shape
    ws = torch.full((max(hip_lib.pram_simple_nms_workspace_bytes(B, h, w), 1),), fill, dtype=torch.uint8, device=s.device)
    out = torch.full_like(s, SENTINEL)
    assert hip_lib.pram_simple_nms_f32(s.data_ptr(), out.data_ptr(), B, h, w, radius, ws.data_ptr(), _st()) == 0
    return out


@pytest.mark.parametrize("radius", D.NMS_RADII)
def test_nms_bit_equal_on_every_case(dev, hip_lib, radius):
    """every case equals the reference bit for bit, through the wrapper and through the entry with a workspace of 0xFF bytes
    (NaN as fp32: a stage that read what it did not write would show), and the frames of a batch equal the frames run alone"""
    from pram_amd import ops
    for name, shape, content in D.nms_cases():
        s = D.nms_map(shape, content, radius)
        want = R.simple_nms(s, radius)
        sd = s.to(dev)
        got = ops.simple_nms(sd, radius)
        assert torch.equal(got.cpu(), want), (name, radius)
        assert torch.equal(_nms_entry(hip_lib, sd, radius, 0xFF), got), (name, radius, "dirty workspace")
        if shape[0] > 1:
            for b in range(shape[0]):
                assert torch.equal(ops.simple_nms(sd[b:b + 1].contiguous(), radius)[0], got[b]), (name, radius, b)


# ------------------------------------------------------------------------------------------------ selection
def _select_entry(hip_lib, case, nms, fill):
    """the C entry on sentinel-filled outputs with a caller-owned workspace prefilled with the byte ``fill``"""
    B, h, w = nms.shape
    k = case.k
    ws = torch.full((max(hip_lib.pram_select_keypoints_workspace_bytes(B, h, w, k), 1),), fill, dtype=torch.uint8, device=nms.device)
    kp = torch.full((B, k, 2), SENTINEL, device=nms.device)
    sc = torch.full((B, k), SENTINEL, device=nms.device)
    cnt = torch.full((B,), -9, dtype=torch.int32, device=nms.device)
    rc = hip_lib.pram_select_keypoints_f32(nms.data_ptr(), B, h, w, float(case.conf_th), case.min_kp, case.border, k, case.fallback_ref,
                                           kp.data_ptr(), sc.data_ptr(), cnt.data_ptr(), ws.data_ptr(), _st())
    assert rc == 0
    return kp.cpu(), sc.cpu(), cnt.cpu()


def _check_selection(case, got, want, tag=""):
    kp, sc, cnt = got
    kps, scs = want
    assert torch.equal(cnt, torch.tensor([len(s) for s in scs], dtype=torch.int32)), (case.name, tag, cnt.tolist(), [len(s) for s in scs])
    for b in range(len(scs)):
        n = len(scs[b])
        assert torch.equal(kp[b, :n], kps[b]), (case.name, tag, b, "keypoints")
        assert torch.equal(sc[b, :n], scs[b]), (case.name, tag, b, "scores")
        assert bool((kp[b, n:] == SENTINEL).all()) and bool((sc[b, n:] == SENTINEL).all()), (case.name, tag, b, "rows beyond counts")


@pytest.fixture(scope="module")
def sel_refs():
    """the reference of every case, computed once and shared (read only)"""
    return {c.name: D.sel_reference(c) for c in SEL}


@pytest.mark.parametrize("case", SEL, ids=lambda c: c.name)
def test_selection_equals_the_reference(dev, hip_lib, sel_refs, case):
    """counts, keypoints and scores in canonical order, and the prefill in every row at and beyond counts[b]: on a zeroed and on a
    0xFF workspace, and through the wrapper"""
    from pram_amd import ops
    nms = case.nms.to(dev)
    want = sel_refs[case.name]
    _check_selection(case, _select_entry(hip_lib, case, nms, 0x00), want, "clean workspace")
    _check_selection(case, _select_entry(hip_lib, case, nms, 0xFF), want, "dirty workspace")
    kp, sc, cnt = ops.select_keypoints(nms, case.conf_th, case.min_kp, case.border, case.k, fallback_ref=case.fallback_ref)
    for b, n in enumerate(cnt.tolist()):
        assert n == len(want[1][b]) and torch.equal(kp[b, :n].cpu(), want[0][b]) and torch.equal(sc[b, :n].cpu(), want[1][b]), (case.name, b)


def test_selection_batch_equals_frames_alone(dev, hip_lib):
    """three frames in different regimes (c <= k, c > k, empty) under fallback_ref = -1: each equals the frame run alone, and
    the reference"""
    case = D.sel_regime_batch()
    nms = case.nms.to(dev)
    kp, sc, cnt = _select_entry(hip_lib, case, nms, 0xFF)
    _check_selection(case, (kp, sc, cnt), D.sel_reference(case))
    for b in range(3):
        kp1, sc1, cnt1 = _select_entry(hip_lib, case, nms[b:b + 1].contiguous(), 0xFF)
        assert int(cnt1[0]) == int(cnt[b]) and torch.equal(kp1[0], kp[b]) and torch.equal(sc1[0], sc[b]), b


# ------------------------------------------------------------------------------------------------ empty extents
@pytest.mark.parametrize("extent", [(0, 5, 7), (2, 0, 7), (2, 5, 0)], ids=["batch=0", "h=0", "w=0"])
def test_empty_extents_return_ok_and_write_nothing(dev, hip_lib, extent):
    B, h, w = extent
    src = torch.full((256,), 0.5, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)

    def fresh():
        return torch.full((256,), SENTINEL, device=dev)

    def untouched(*ts):
        return all(bool((t == SENTINEL).all()) for t in ts)

    out = fresh()
    assert hip_lib.pram_score_map_f32(src.data_ptr(), out.data_ptr(), B, h, w, _st()) == 0 and untouched(out)
    out = fresh()
    for radius in D.NMS_RADII:
        assert hip_lib.pram_simple_nms_f32(src.data_ptr(), out.data_ptr(), B, h, w, radius, ws.data_ptr(), _st()) == 0, radius
    assert untouched(out) and hip_lib.pram_simple_nms_workspace_bytes(B, h, w) == 0
    kp, sc, cnt = fresh(), fresh(), torch.full((8,), -9, dtype=torch.int32, device=dev)
    for k in (3, 9000):
        for ref in (-1, 0) if B else (-1,):
            assert hip_lib.pram_select_keypoints_f32(src.data_ptr(), B, h, w, D.CONF_TH, 10, 0, k, ref, kp.data_ptr(), sc.data_ptr(),
                                                     cnt.data_ptr(), ws.data_ptr(), _st()) == 0, (k, ref)
    assert untouched(kp, sc) and bool((cnt == -9).all())
    for c in (4, 0):
        out = fresh()
        assert hip_lib.pram_nhwc_to_nchw_f32(src.data_ptr(), out.data_ptr(), B, h, w, c, _st()) == 0 and untouched(out), c
    out = fresh()
    assert hip_lib.pram_nhwc_to_nchw_f32(src.data_ptr(), out.data_ptr(), 2, 3, 3, 0, _st()) == 0 and untouched(out)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ score lookup
def _lookup(hip_lib, dev, maps, kpts, lens):
    """pram_score_lookup_f32 with kpts and out in the middle of larger sentinel-filled tensors (LOOKUP_GUARD rows on each side,
    more than a launch can overrun): -> (out [B, N], the guards kept their bits)"""
    Bm, h, w = maps.shape
    B, N, _ = kpts.shape
    G = D.LOOKUP_GUARD
    kbuf = torch.full((G + B * N + G, 2), 3.0, device=dev)          # a guard row is a valid keypoint: a stray read finds (3, 3)
    kbuf[G:G + B * N] = kpts.reshape(B * N, 2).to(dev)
    obuf = torch.full((G + B * N + G,), SENTINEL, device=dev)
    kv, ov = kbuf[G:G + B * N], obuf[G:G + B * N]
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    rc = hip_lib.pram_score_lookup_f32(maps.data_ptr(), h * w if Bm > 1 else 0, h, w, kv.data_ptr(), None if ln is None else ln.data_ptr(),
                                       B, N, ov.data_ptr(), _st())
    assert rc == 0
    guards = bool((obuf[:G] == SENTINEL).all()) and bool((obuf[G + B * N:] == SENTINEL).all()) and bool((kbuf[:G] == 3.0).all()) and \
        bool((kbuf[G + B * N:] == 3.0).all())
    return ov.view(B, N).cpu(), guards


def test_score_lookup_clamps_lengths_and_tests_coordinates(dev, hip_lib):
    """lengths above n_max and below 0 behave as n_max and 0, nothing is written past a frame's rows or the tensor; keypoints
    outside the map (and NaN) score 0 and their in-range neighbours are untouched"""
    from pram_amd import weights as W
    h, w, N = 13, 17, 40
    maps = W.uniform(8600, "lk/m", (2, h, w), 0.5, 1.0).contiguous()
    kpts = torch.stack([W.uniform(8600, "lk/x", (2, N), 0.0, float(w)), W.uniform(8600, "lk/y", (2, N), 0.0, float(h))], -1).contiguous()
    md = maps.to(dev)

    def want(lens):
        out = torch.full((2, N), SENTINEL)
        for b in range(2):
            for n in range(max(0, min(lens[b], N))):
                x, y = float(kpts[b, n, 0]), float(kpts[b, n, 1])
                out[b, n] = maps[b, int(y), int(x)] if 0 <= x < w and 0 <= y < h else 0.0
        return out

    for lens in ([N, N], [N + 5, 7], [7, N + 5], [-3, N], [N, -3], [N + 5, -3], [0, N + 300]):
        got, guards = _lookup(hip_lib, dev, md, kpts, lens)
        assert guards, lens
        assert torch.equal(got, want(lens)), lens
    got, guards = _lookup(hip_lib, dev, md, kpts, None)
    assert guards and torch.equal(got, want([N, N]))

    nan = float("nan")
    outside = [(-1.0, 0.0), (float(w), 0.0), (0.0, float(h)), (nan, 0.0), (0.0, nan), (1e9, 0.0), (0.0, 1e9), (-1e9, -1e9), (-0.5, 2.0),
               (2.0, -1e-3), (float("inf"), 1.0), (1.0, float("-inf"))]
    for j, (x, y) in enumerate(outside):
        kpts[j % 2, 3 * j + 1] = torch.tensor([x, y])
    edge = [(float(w) - 0.25, float(h) - 0.25), (0.0, 0.0), (np.nextafter(np.float32(w), np.float32(0)), 0.5)]      # still inside
    for j, (x, y) in enumerate(edge):
        kpts[1, 37 + j] = torch.tensor([float(x), float(y)])
    full = want([N, N])
    assert int((full == 0).sum()) == len(outside) and float(full[1, 37]) == float(maps[1, h - 1, w - 1])
    for lens in (None, [N, N], [N + 5, N - 2]):
        got, guards = _lookup(hip_lib, dev, md, kpts, lens)
        assert guards and torch.equal(got, want(lens or [N, N])), lens
    one, guards = _lookup(hip_lib, dev, md[:1].contiguous(), kpts[1:], [N + 5])      # map_stride = 0: one map for every set
    exp = want([0, N])[1].clone()
    for n in range(N):
        x, y = float(kpts[1, n, 0]), float(kpts[1, n, 1])
        exp[n] = maps[0, int(y), int(x)] if 0 <= x < w and 0 <= y < h else 0.0
    assert guards and torch.equal(one[0], exp)
