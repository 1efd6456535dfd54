"""GPU (MI355X): the descriptor head's last two layers computed only at the map pixels the keypoints sample (row list -> gathered
3x3 -> 1x1 + normalize on the rows -> sampling through the list) against the dense layers + sample_nhwc: the same bits at the op,
the model and the pipeline, a deterministic list, and a skip rule that reads nothing that was not written."""
import pytest
import torch

from pram_amd import ops, weights as W
from tests import helpers as H

pytestmark = pytest.mark.gpu

FH, FW, CIN, S = 24, 40, 256, 4


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def head(dev):
    """map [2, 24, 40, 256], the 3x3 and the 1x1 of the head, and the dense descriptor map (computed once, shared)"""
    x = W.normal(51, "sd/x", (2, FH, FW, CIN), 1.0).to(dev)
    w3 = W.normal(51, "sd/w3", (256, 3, 3, CIN), (9 * CIN) ** -0.5).to(dev)
    b3 = W.normal(51, "sd/b3", (256,), 0.1).to(dev)
    w1 = W.normal(51, "sd/w1", (128, 1, 1, 256), 256 ** -0.5).to(dev)
    b1 = W.normal(51, "sd/b1", (128,), 0.1).to(dev)
    dm = ops.conv2d_nhwc(ops.conv2d_nhwc(x, w3, b3, ks=3, precision="x3"), w1, b1, ks=1, precision="x3", l2norm=True)
    return dict(x=x, w3=w3, b3=b3, w1=w1, b1=b1, dm=dm)


def _keypoints(k, seed=0):
    """[2, k, 2] integer (x, y) image coordinates at stride 4: the four image corners (a sampling corner falls outside the map on
    every side), duplicates of them and of a random keypoint, random ones for the rest"""
    g = torch.Generator().manual_seed(1234 + seed)
    kp = torch.stack([torch.randint(0, FW * S, (2, k), generator=g), torch.randint(0, FH * S, (2, k), generator=g)], -1).float()
    edge = torch.tensor([[0., 0.], [FW * S - 1., FH * S - 1.], [0., FH * S - 1.], [FW * S - 1., 0.]])
    kp[:, :4] = edge
    kp[:, 4:8] = edge              # duplicates
    kp[:, 9] = kp[:, 8]
    kp[1, 20] = kp[1, 30]
    return kp


def _corner_pixels(kp, n):
    """the set of valid corner pixels of the first n keypoints of one frame: sample_descriptors' arithmetic in fp32 on the CPU"""
    kx, ky = kp[:n, 0], kp[:n, 1]
    half = torch.tensor(S * 0.5)
    gx = ((kx - half) + 0.5) / (FW * S - half - 0.5) * 2 - 1
    gy = ((ky - half) + 0.5) / (FH * S - half - 0.5) * 2 - 1
    x0 = torch.floor(((gx + 1) / 2) * (FW - 1)).long()
    y0 = torch.floor(((gy + 1) / 2) * (FH - 1)).long()
    px = set()
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < FW) & (yy >= 0) & (yy < FH)
            px |= set((yy[ok] * FW + xx[ok]).tolist())
    return px


def _poison(dev, nbytes):
    """Best effort only: leave freed blocks full of 1e30 in the caching allocator, which the next torch.empty of that size is likely
    (not certain) to hand out, so that a read of an unwritten row would trip the range guard or show in the result.  The check that
    does not depend on the allocator is test_skipped_tiles_are_neither_written_nor_read."""
    t = torch.full((nbytes // 4,), 1e30, device=dev)
    del t


@pytest.mark.parametrize("counts", [[64, 0], [1, 37]])
def test_sparse_descriptors_equal_dense(dev, head, counts):
    h = head
    k = 64
    kp = _keypoints(k).to(dev)
    lens = torch.tensor(counts, device=dev, dtype=torch.int32)
    want = ops.sample_nhwc(h["dm"], kp, lens, S, True)
    rlen = ops.sparse_desc_rows(k, FH, FW)
    assert rlen == 256                                      # 4 k = 256 of 960 pixels: the sparse form
    ops.x3_range_exceeded(dev)                              # clear
    _poison(dev, 2 * rlen * 256 * 4)
    got, rows, n_rows, pix2row = ops.sparse_descriptors(h["x"], h["w3"], h["b3"], h["w1"], h["b1"], kp, lens, S, rlen, want_parts=True)
    assert not ops.x3_range_exceeded(dev)
    assert torch.equal(got, want)
    for b, n in enumerate(counts):
        assert bool((got[b, n:] == 0).all())                # rows beyond counts stay zero
        assert int(n_rows[b]) == len(_corner_pixels(kp[b].cpu(), n))
    assert torch.equal(ops.sampled_descriptors(h["x"], h["w3"], h["b3"], h["w1"], h["b1"], kp, lens, S), want)


@pytest.mark.parametrize("counts", [[64, 0], [1, 37]])
def test_long_lists_take_the_dense_path_and_are_equal(dev, head, counts, monkeypatch):
    """4 k >= fh fw: sampled_descriptors must not build a list"""
    h = head
    k = 256
    assert 4 * k >= FH * FW and ops.sparse_desc_rows(k, FH, FW) == 0
    kp = torch.cat([_keypoints(64, seed=j) for j in range(4)], 1).to(dev)
    lens = torch.tensor(counts, device=dev, dtype=torch.int32)

    def refuse(*a, **kw):
        raise AssertionError("the sparse form was taken")
    monkeypatch.setattr(ops, "sparse_descriptors", refuse)
    got = ops.sampled_descriptors(h["x"], h["w3"], h["b3"], h["w1"], h["b1"], kp, lens, S)
    assert torch.equal(got, ops.sample_nhwc(h["dm"], kp, lens, S, True))


def test_row_list_kernel(dev, head):
    """the listed pixels are the valid corners, ascending and live-first; pix2row inverts the list; two runs give one layout"""
    from pram_amd import _lib
    L = _lib.load()
    k, rlen = 64, 256
    kp = _keypoints(k).to(dev)
    for counts in ([64, 0], [1, 37], [64, 64]):
        lens = torch.tensor(counts, device=dev, dtype=torch.int32)
        runs = []
        for _ in range(2):
            rows = torch.full((2, rlen), -7, device=dev, dtype=torch.int32)
            n_rows = torch.full((2,), -7, device=dev, dtype=torch.int32)
            p2r = torch.full((2, FH * FW), -7, device=dev, dtype=torch.int32)
            _lib.check(L.pram_sfd2_row_list(kp.data_ptr(), lens.data_ptr(), 2, k, FH, FW, S, rows.data_ptr(), n_rows.data_ptr(),
                                            p2r.data_ptr(), rlen, None), "pram_sfd2_row_list")
            runs.append((rows.cpu(), n_rows.cpu(), p2r.cpu()))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        rows, n_rows, p2r = runs[0]
        for b, n in enumerate(counts):
            want = sorted(_corner_pixels(kp[b].cpu(), n))
            m = int(n_rows[b])
            assert rows[b, :m].tolist() == want             # the set, ascending, live first
            assert bool((rows[b, m:] == -1).all())
            assert p2r[b, rows[b, :m].long()].tolist() == list(range(m))
            rest = torch.ones(FH * FW, dtype=torch.bool)
            rest[rows[b, :m].long()] = False
            assert bool((p2r[b, rest] == -7).all())         # nothing else is written


def test_skipped_tiles_are_neither_written_nor_read(dev, head):
    """one frame with a single keypoint, one with none, four tiles per frame: one tile runs, seven are skipped.  The rows of
    skipped tiles keep the poison they were allocated with through both layers, the guard does not trip, the result is dense's."""
    from pram_amd import _lib
    L = _lib.load()
    h = head
    k, rlen = 64, 1024
    kp = _keypoints(k).to(dev)
    kp[0, 0] = torch.tensor([37., 50.])                     # an interior keypoint: four live rows
    lens = torch.tensor([1, 0], device=dev, dtype=torch.int32)
    want = ops.sample_nhwc(h["dm"], kp, lens, S, True)
    ops.x3_range_exceeded(dev)
    got, rows, n_rows, _ = ops.sparse_descriptors(h["x"], h["w3"], h["b3"], h["w1"], h["b1"], kp, lens, S, rlen, want_parts=True)
    assert not ops.x3_range_exceeded(dev)
    assert n_rows.tolist() == [4, 0] and torch.equal(got, want)
    # the two layers by hand on poisoned buffers
    mid = torch.full((2 * rlen, 256), 1e30, device=dev)
    out = torch.full((2 * rlen, 128), 1e30, device=dev)
    wh, wl, ws = ops.split_weight(h["w3"])
    _lib.check(L.pram_conv3x3_rows_x3_f32(h["x"].data_ptr(), 2, FH, FW, CIN, wh.data_ptr(), wl.data_ptr(), ws, h["b3"].data_ptr(),
                                          rows.data_ptr(), n_rows.data_ptr(), rlen, mid.data_ptr(), 256, 0, None), "rows 3x3")
    wh, wl, ws = ops.split_weight(h["w1"])
    _lib.check(L.pram_conv1x1_rows_x3_l2norm_f32(mid.data_ptr(), 2, rlen, 256, wh.data_ptr(), wl.data_ptr(), ws, h["b1"].data_ptr(),
                                                 n_rows.data_ptr(), out.data_ptr(), 128, None), "rows 1x1")
    assert not ops.x3_range_exceeded(dev)                   # 1e30 * 16 would have tripped it
    live = torch.zeros(2 * rlen, dtype=torch.bool, device=dev)
    live[:ops.SPARSE_ROWS_TILE] = True                      # frame 0's first tile: four live rows, the rest repeat the last one
    assert bool((mid[~live] == 1e30).all()) and bool((out[~live] == 1e30).all())
    assert bool(torch.isfinite(mid[live]).all()) and bool((mid[live].abs() < 1e3).all())
    px = rows[0, :4].long()
    dense_mid = ops.conv2d_nhwc(h["x"], h["w3"], h["b3"], ks=3, precision="x3")
    assert torch.equal(mid[:4], dense_mid[0].reshape(-1, 256)[px])
    assert torch.equal(out[:4], h["dm"][0].reshape(-1, 128)[px])
    assert torch.equal(mid[4:256], mid[3:4].expand(252, 256)) and torch.equal(out[4:256], out[3:4].expand(252, 128))


# ------------------------------------------------------------------------------------------------ model and pipeline
def _models(dev):
    from pram_amd.nets.gml import GML
    from pram_amd.nets.load_segnet import load_segnet
    from pram_amd.nets.sfd2 import ResNet4x
    sfd2, seg, gml = ResNet4x(), load_segnet('segnetvit', 113, 256, 15, 1024), GML({})
    for m, sd in ((sfd2, H.sfd2_sd()), (seg, H.segnet_sd(113)), (gml, H.gml_sd())):
        m.load_state_dict(sd, strict=True)
        m.to(dev).eval()
    return sfd2, seg, gml


@pytest.fixture(scope="module")
def models(dev):
    return _models(dev)


def _frames(dev):
    return torch.stack([W.synthetic_image(1, 96, 128), W.synthetic_image(2, 96, 128)]).to(dev)


def _count_sparse(monkeypatch):
    calls = []
    real = ops.sparse_descriptors

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "sparse_descriptors", counted)
    return calls


# 128 keypoints on a 24 x 32 map list 512 of 768 pixels: where the shipped crossover sends that to the dense layers the case is also
# run with the crossover lifted, and with 64 keypoints (256 of 768 pixels), which is sparse at the shipped crossover
CASES = [(128, None), (128, 1.0), (64, None)]


@pytest.mark.parametrize("k,fraction", CASES)
def test_extract_batched_sparse_equals_default(dev, models, k, fraction, monkeypatch):
    sfd2 = models[0]
    if fraction is not None:
        monkeypatch.setattr(ops, "SPARSE_DESC_MAX_FRACTION", fraction)
    calls = _count_sparse(monkeypatch)
    img = _frames(dev)
    cfg = {'min_keypoints': 8, 'max_keypoints': k}
    want = sfd2.extract_batched(img, cfg)
    assert not calls and want['desc_map'] is not None
    got = sfd2.extract_batched(img, cfg, dense_desc=False)
    assert got['desc_map'] is None
    assert len(calls) == (1 if ops.sparse_desc_rows(k, 24, 32) else 0)
    if fraction == 1.0 or k == 64:
        assert calls
    for key in ('descriptors', 'keypoints', 'scores', 'counts'):
        assert torch.equal(got[key], want[key]), key


@pytest.mark.parametrize("k,fraction", CASES)
def test_pipeline_record_sparse_equals_dense_eager_and_graphed(dev, models, k, fraction, monkeypatch):
    from pram_amd.pipeline import GraphedPipeline, QueryPipeline
    sfd2, seg, gml = models
    if fraction is not None:
        monkeypatch.setattr(ops, "SPARSE_DESC_MAX_FRACTION", fraction)
    img = _frames(dev)
    dense = QueryPipeline(sfd2, seg, gml, max_keypoints=k, min_keypoints=8, dense_desc=True)
    pipe = QueryPipeline(sfd2, seg, gml, max_keypoints=k, min_keypoints=8)
    assert pipe.dense_desc is False                         # the default: the pipeline does not read the map
    ex = sfd2.extract_batched(img, pipe.cfg)
    ref = {"descriptors": ex["descriptors"].flip(1).contiguous(), "keypoints": ex["keypoints"].flip(1).contiguous(),
           "scores": ex["scores"].flip(1).contiguous()}
    calls = _count_sparse(monkeypatch)
    want = QueryPipeline.pack_record(dense.run(img, ref, stages="erm")).clone()
    assert not calls
    got = QueryPipeline.pack_record(pipe.run(img, ref, stages="erm")).clone()
    assert torch.equal(got, want)
    if fraction == 1.0 or k == 64:
        assert calls
    g = GraphedPipeline(pipe, img, ref, stages="erm", record=True)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g.record, want)
