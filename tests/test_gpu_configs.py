"""GPU (MI355X): the BASELINE.json configurations at THEIR sizes on the HIP path, against the oracle.

  C3  7Scenes full pipeline, B = 16 queries of 640x480 / 2048 keypoints through QueryPipeline.run, AdaGML at 2048 x 2048;
  C4  Cambridge: 4096 keypoints, nc161, fp32-class path (SegNetViT N = 4096, GML 4096 x 4096, SFD2 extraction with k = 4096);
  C5  Aachen: fp16 MFMA path, 4096 keypoints, nc513 (own documented tolerance).

Tolerances as everywhere: fp32-class paths 1e-3 abs on floats, indices exact (an index may only differ where the very
same candidate sits on the `score > p` acceptance threshold to 1e-5 — reported, none expected on these inputs);
the C5 path has its own looser bars, written next to the check."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from pram_amd import weights as W
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    torch.set_num_threads(max(1, min(32, len(__import__("os").sched_getaffinity(0)))))
    return torch.device("cuda:0")


def _to(data, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}


def _segnet(dev, C):
    from pram_amd.nets.load_segnet import load_segnet
    m = load_segnet('segnetvit', C, 256, 15, 1024)
    m.load_state_dict(H.segnet_sd(C), strict=True)
    return m.to(dev).eval()


def _tokens(N, idx=0):
    d, k, _ = W.synthetic_tokens(idx, N)
    return d[None], k[None]


def test_c4_segnetvit_4096_nc161_vs_oracle(dev):
    """C4: the recogniser at 4096 tokens, 161 classes, on the default (fp32-class) path."""
    desc, kp = _tokens(4096)
    ref = R.segnetvit_forward(H.segnet_sd(161), desc, kp, (1, 3, 480, 640))
    out = _segnet(dev, 161)({"seg_descriptors": desc.to(dev), "keypoints": kp.to(dev), "image": torch.empty(1, 3, 480, 640)})["prediction"]
    d = H.maxdiff(out, ref)
    agree = (out.argmax(-1).cpu() == ref.argmax(-1)).float().mean().item()
    print(f"C4 segnetvit N=4096 nc161: max |logit - oracle| = {d:.2e}, argmax agreement {agree:.5f}")
    assert tuple(out.shape) == (1, 4096, 161) and d < 1e-3 and agree >= 0.999


def test_c4_gml_4096x4096_vs_oracle(dev):
    from pram_amd.nets.gml import GML
    data, _ = H.pair_data(2, 4096, 4096)
    ref = R.gml_produce_matches(H.gml_sd(), data, p=0.2)
    net = GML({})
    net.load_state_dict(H.gml_sd(), strict=True)
    r = net.to(dev).eval()(_to(data, dev))
    d = H.maxdiff(r["matching_scores0"], ref["matching_scores0"])
    mism = (r["matches0"].cpu() != ref["matches0"]).sum().item()
    mism1 = (r["matches1"].cpu() != ref["matches1"]).sum().item()
    print(f"C4 gml 4096x4096: score diff {d:.2e}, mismatching indices {mism} / {mism1}, matches {(ref['matches0'] >= 0).sum().item()}")
    assert d < 1e-3 and mism == 0 and mism1 == 0


def test_c3_adagml_2048x2048_vs_oracle(dev):
    """C3 names AdaGML: stop layer, surviving token ids and matches at the configuration's 2048 x 2048."""
    from pram_amd.nets.adagml import AdaGML
    data, _ = H.pair_data(6, 2048, 2048)
    po = {}
    ref = R.adagml_produce_matches(H.adagml_sd(), data, p=0.2, probes=po)
    net = AdaGML({})
    net.load_state_dict(H.adagml_sd(), strict=True)
    pg = {}
    r = net.to(dev).eval().produce_matches(_to(data, dev), p=0.2, probes=pg)
    lens = pg["lens"].tolist()
    print(f"C3 adagml 2048x2048: oracle stop layer {po['stop_layer']} sizes {po['sizes']}; hip stop {int(pg['stop_layer'][0])} survivors {lens}; "
          f"matches {(ref['matches0'] >= 0).sum().item()}")
    assert int(pg["stop_layer"][0]) == po["stop_layer"]
    assert torch.equal(pg["ind"][0, :lens[0]].cpu().long(), po["ind0"]) and torch.equal(pg["ind"][1, :lens[1]].cpu().long(), po["ind1"])
    assert torch.equal(r["matches0"].cpu(), ref["matches0"])
    assert H.maxdiff(r["matching_scores0"], ref["matching_scores0"]) < 1e-3


def test_c4_sfd2_extraction_k4096_vs_oracle(dev):
    """C4: 4096 keypoints asked of a 640x480 frame: same keypoint SET as the oracle (shortfall reported, never padded),
    scores 1e-5, descriptors 1e-3 at the keypoints both agree on."""
    from pram_amd.nets.sfd2 import ResNet4x
    net = ResNet4x()
    net.load_state_dict(H.sfd2_sd(), strict=True)
    net = net.to(dev).eval()
    imgs = torch.stack([W.synthetic_image(0), W.synthetic_image(5)])
    cfg = {"min_keypoints": 128, "max_keypoints": 4096}
    r = net.extract_batched(imgs.to(dev), cfg, per_image_fallback=True)
    counts = r["counts"].tolist()
    for b in range(2):
        o = R.sfd2_extract_local_global(H.sfd2_sd(), imgs[b:b + 1], max_keypoints=4096, min_keypoints=128, per_image_fallback=True)
        okp, osc = o["keypoints"][0], o["scores"][0]
        kp, sc = r["keypoints"][b, :counts[b]].cpu(), r["scores"][b, :counts[b]].cpu()
        want = {(int(x), int(y)): i for i, (x, y) in enumerate(okp.tolist())}
        got = {(int(x), int(y)): i for i, (x, y) in enumerate(kp.tolist())}
        common = sorted(set(want) & set(got))
        print(f"C4 sfd2 frame {b}: {counts[b]} keypoints (asked 4096, shortfall {4096 - counts[b]}), oracle {len(okp)}, common {len(common)}")
        assert counts[b] == len(okp)
        # a candidate at the very end of the top-k list may swap with its neighbour (scores equal to ~1e-7): allow 2 of 4096
        assert len(common) >= len(okp) - 2
        gi = torch.tensor([got[c] for c in common])
        wi = torch.tensor([want[c] for c in common])
        assert float((sc[gi] - osc[wi]).abs().max()) < 1e-5
        dd = (r["descriptors"][b, :counts[b]].cpu()[gi] - o["descriptors"][0].t()[wi]).abs().max().item()
        assert dd < 1e-3, dd


def test_c5_fp16_path_nc513_4096(dev):
    """C5: 'fp16 MFMA path', 4096 keypoints, 513 classes.  Own documented tolerance (single fp16 product per MAC), set at 1.5 x the
    measurement (3.3-4.05e-2 from the fp32 oracle, arg-max agreement 0.9961-0.9971): logits
    within 6.1e-2, arg-max agreement >= 99.42 % (= bench.F16_BARS, what alt.c5_f16.parity gates on); NOT the fp32 parity configuration."""
    desc, kp = _tokens(4096, idx=2)
    ref = R.segnetvit_forward(H.segnet_sd(513), desc, kp, (1, 3, 480, 640))
    net = _segnet(dev, 513).set_precision("f16")
    out = net({"seg_descriptors": desc.to(dev), "keypoints": kp.to(dev), "image": torch.empty(1, 3, 480, 640)})["prediction"]
    d = H.maxdiff(out, ref)
    agree = (out.argmax(-1).cpu() == ref.argmax(-1)).float().mean().item()
    net.set_precision(None)
    d3 = H.maxdiff(net({"seg_descriptors": desc.to(dev), "keypoints": kp.to(dev), "image": torch.empty(1, 3, 480, 640)})["prediction"], ref)
    print(f"C5 segnetvit N=4096 nc513: fp16 path |logit - oracle| {d:.2e}, argmax agreement {agree:.4f}; default path {d3:.2e}")
    assert tuple(out.shape) == (1, 4096, 513) and d < 6.1e-2 and agree >= 0.9942
    assert d3 < 1e-3


def test_c3_pipeline_b16_full_size(dev):
    """C2/C3 at the benchmark's size: 16 queries of 640x480, 2048 keypoints, recogniser + GML against 2048-keypoint
    reference sets, one QueryPipeline.run.  Properties of the record, and two of the sixteen queries re-run alone
    (B = 1) must reproduce their batched result bit for bit."""
    import bench
    from pram_amd.pipeline import QueryPipeline
    sfd2, seg, gml, sds = bench.build_models(dev, "gml", 113)
    pipe = QueryPipeline(sfd2, seg, gml, max_keypoints=2048, min_keypoints=128)
    B = 16
    images = torch.stack([W.synthetic_image(i) for i in range(B)]).to(dev)
    ex = sfd2.extract_batched(images, pipe.cfg)
    counts = ex["counts"].tolist()
    sd = W.calibrate_matcher_input(sds["gml"], ex["descriptors"][0, :counts[0]])
    gml.load_state_dict(sd, strict=True)
    gml.to(dev).eval()
    ref, gt = bench.make_reference_sets(ex["descriptors"], ex["keypoints"], ex["scores"], counts, 5000)
    out = pipe.run(images, ref)
    rec = QueryPipeline.pack_record(out)
    assert tuple(rec.shape) == (B, 2048, 6) and out["counts"].tolist() == counts and all(c == 2048 for c in counts)
    m0, s0 = out["matches0"], out["matching_scores0"]
    valid = m0 >= 0
    assert int(valid.sum()) > 0.3 * int((gt >= 0).sum())                 # the planted twins are found ...
    assert float(((m0 == gt) & valid).sum()) / float(valid.sum()) > 0.99  # ... and what is found is right
    assert bool((s0[valid] > 0.2).all()) and bool((s0 >= 0).all()) and bool((m0[valid] < 2048).all())
    for b in range(B):                                                   # a reference keypoint is matched at most once
        mb = m0[b][valid[b]]
        assert mb.unique().numel() == mb.numel()
    lm = out["landmark"]
    assert int(lm.min()) >= -1 and int(lm.max()) < 112 and tuple(out["prediction"].shape) == (B, 2048, 113)
    assert bool(torch.isfinite(out["prediction"]).all())
    for b in (3, 11):
        solo = pipe.run(images[b:b + 1], {k: v[b:b + 1] for k, v in ref.items()})
        for key in ("keypoints", "scores", "descriptors", "prediction", "matches0", "matching_scores0", "landmark"):
            assert torch.equal(out[key][b], solo[key][0]), (b, key)


def test_c5_fp16_pipeline_discrete_outputs_as_fractions(dev):
    """C5 end to end on the fp16 MFMA path (one 640 x 480 frame, 4096 keypoints, nc513, GML against a 4096-keypoint reference set)
    through bench.parity_gate(f16=True): the recogniser inside its documented bars, and the path's DISCRETE outputs — which keypoints,
    which match indices — gated as agreement FRACTIONS with the fp32 oracle (bench.F16_BARS: 1.5 x the measured deficit), not as
    booleans that cannot say whether one or a thousand differ."""
    import bench
    from pram_amd import ops
    job = bench.Job(dev, 0, 1, 0, 1, "gml", 4096, 513, "erm", 1, False, precision="f16")
    with torch.no_grad(), ops.precision_scope("f16"):
        pq = bench.parity_gate(job.pipe, job.sds, "gml", job.images, job.ref, 4096, queries=(0,), f16=True)
    print({k: v for k, v in pq.items() if k != "per_query"})
    assert pq["ok"], pq
    assert pq["keypoint_set_overlap_min"] >= bench.F16_BARS["kp_overlap"] and pq["match_index_agreement_min"] >= bench.F16_BARS["match_agree"]
    assert pq["logits_maxdiff_max"] < bench.F16_BARS["logits"] and pq["argmax_agreement_min"] >= bench.F16_BARS["argmax"]
    if ops.x3_launched(dev):
        assert not ops.x3_range_exceeded(dev)
