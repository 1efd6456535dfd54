"""GPU: the query pre-filter (csrc/prefilter.hip) and the Localizer (pram_amd.localization.localizer) against the numpy
restatement tests/localizer_ref.py: the kernel alone as bits, the cases pinned by the reference through prefilter_queries,
run_features on track_ref.sequence_scene against Tracker.run called by hand on the restatement's filtered arrays, run from images
against the three stages called by hand, and the evaluation helpers on the scene's planted cameras."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cand_ref as CR
from tests import helpers as H
from tests import localizer_ref as LR
from tests import pose_ref as PR
from tests import refine_ref as RR
from tests import track_ref as TR

pytestmark = pytest.mark.gpu

ROW_KEYS = ("keypoints", "scores", "descriptors", "logits", "seg_ids")
D = 128


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    t = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(t).reshape(-1).view(np.uint8)


def _random_words(rng, shape):
    """Random bits in 32-bit words, none of which reads as a float32 infinity or NaN (tests/test_gpu_track.py::_random_bytes: the
    buffers go back to the caching allocator)."""
    words = rng.integers(0, 2 ** 32, shape, dtype=np.uint32)
    words[(words & 0x7F800000) == 0x7F800000] &= np.uint32(0xFF7FFFFF)
    return words


def _inputs(rng, B, N, n_class, counts, masks):
    """Random bits in every row of every input, inside and beyond counts[b]; the masks take any non-zero value for 'kept' and
    random values beyond the count.  -> (host arrays as 32-bit words, device tensors)."""
    host = {"keypoints": _random_words(rng, (B, N, 2)), "scores": _random_words(rng, (B, N)), "descriptors": _random_words(rng, (B, N, D)),
            "logits": _random_words(rng, (B, N, n_class)), "seg_ids": rng.integers(-1, 2 ** 20, (B, N)).astype(np.int32)}
    mask = np.where(np.asarray(masks, dtype=bool), rng.integers(1, 2 ** 31, (B, N)), 0).astype(np.int32)
    for b in range(B):
        mask[b, counts[b]:] = rng.integers(-5, 5, N - counts[b])
    host["mask"] = mask
    return host


def _call(dev, host, counts, n_non_bg, enable):
    from pram_amd import ops
    f32 = lambda k: torch.from_numpy(host[k].view(np.float32)).to(dev)
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)
    args = [f32("keypoints"), f32("scores"), f32("descriptors"), f32("logits"), i32(host["seg_ids"]), i32(host["mask"]), i32(n_non_bg), i32(counts)]
    before = [a.clone() for a in args]
    out = ops.query_prefilter(*args, enable)
    again = ops.query_prefilter(*args, enable)
    for k in out:
        assert np.array_equal(_bits(out[k]), _bits(again[k])), (k, "two calls differ")
    for a, b in zip(args, before):
        assert np.array_equal(_bits(a), _bits(b)), "an input was written"
    return out


def _check(out, host, counts, n_non_bg, enable, what):
    B, N = host["scores"].shape
    want = LR.prefilter_batch({k: host[k] for k in ROW_KEYS[:4]}, counts, 0.95 if enable else 0.0,
                              masks=np.stack([host["mask"][b] != 0 for b in range(B)]) if B else np.zeros((0, N), bool), seg_ids=host["seg_ids"],
                              n_non_bg=n_non_bg)
    for k in ROW_KEYS + ("counts", "kept", "filtered"):
        got = out[k]
        assert tuple(got.shape) == want[k].shape, (what, k)
        assert np.array_equal(_bits(got), _bits(want[k])), (what, k)
    return want


@pytest.mark.parametrize("n_class", [29, 113])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 600])
def test_prefilter_kernel_bit_exact(dev, N, n_class):
    """Every output as bits against the restatement: B = 0, 1 and 5; counts 0, 1 and N; masks all-kept, none-kept (the filter does
    not fire), alternating, a single survivor in the last row (not firing, and firing on a count handed to the entry); the filter
    off (th = 0); random bits beyond counts[b] in every input; two calls bit-equal; the inputs untouched."""
    rng = np.random.default_rng(1000 * N + n_class)
    fired = kept_all = 0
    for enable in (True, False):
        # B = 5, full queries: one mask kind per query
        kinds = np.zeros((5, N), dtype=bool)
        kinds[0] = True
        kinds[2, ::2] = True
        kinds[3, N - 1] = kinds[4, N - 1] = True
        counts = [N] * 5
        nnb = kinds.sum(1)
        nnb[4] = N      # the count the decision is taken on: query 4 fires and keeps its last row alone
        host = _inputs(rng, 5, N, n_class, counts, kinds)
        want = _check(_call(dev, host, counts, nnb, enable), host, counts, nnb, enable, f"kinds N={N} enable={enable}")
        if enable:
            assert want["filtered"].tolist() == [1, 0, 1, int(N <= 2), 1] and want["counts"].tolist() == [N, N, (N + 1) // 2, 1 if N <= 2 else N, 1]
            assert want["kept"][4, 0] == N - 1
        else:
            assert not want["filtered"].any() and (want["counts"] == N).all()
        # B = 5, ragged: counts 0, 1, N and two in between, seeded masks on either side of 40 %
        counts = [0, 1, N, max(N - 1, 0), N // 2]
        masks = rng.uniform(0, 1, (5, N)) < np.array([0.5, 1.0, 0.5, 0.3, 0.45])[:, None]
        nnb = [int(masks[b, :counts[b]].sum()) for b in range(5)]
        host = _inputs(rng, 5, N, n_class, counts, masks)
        want = _check(_call(dev, host, counts, nnb, enable), host, counts, nnb, enable, f"ragged N={N} enable={enable}")
        assert want["filtered"][0] == int(enable) and want["counts"][0] == 0      # an empty query fires
        fired, kept_all = fired + int(want["filtered"].sum()), kept_all + int((want["filtered"] == 0).sum())
        # B = 1 and B = 0
        masks = rng.uniform(0, 1, (1, N)) < 0.6
        host = _inputs(rng, 1, N, n_class, [N], masks)
        _check(_call(dev, host, [N], [int(masks.sum())], enable), host, [N], [int(masks.sum())], enable, f"one N={N} enable={enable}")
        host = _inputs(rng, 0, N, n_class, [], np.zeros((0, N), bool))
        out = _check(_call(dev, host, [], [], enable), host, [], [], enable, f"empty N={N}")
        assert out["counts"].shape == (0,)
    assert fired >= 2 and kept_all >= 5


def test_prefilter_kernel_special_values_and_out_of_range_counts(dev):
    """NaN payloads and negative zeros survive in kept rows; counts beyond N and below 0 are clamped; N = 0 launches nothing."""
    from pram_amd import ops
    rng = np.random.default_rng(77)
    B, N, n_class = 3, 70, 29
    counts = [N + 9, -4, 33]
    masks = rng.uniform(0, 1, (B, N)) < 0.6
    host = _inputs(rng, B, N, n_class, [N, 0, 33], masks)
    for k in ("keypoints", "scores", "descriptors", "logits"):
        flat = host[k].reshape(B, N, -1)
        flat[:, ::3, 0] = 0x7FC00123      # a quiet NaN with a payload
        flat[:, 1::3, -1] = 0xFFA00001    # a signalling NaN, sign set
        flat[:, 2::3, 0] = 0x80000000     # -0.0
    nnb = [int(masks[0].sum()), 0, int(masks[2, :33].sum())]
    out = _call(dev, host, counts, nnb, True)
    want = _check(out, host, [N, 0, 33], nnb, True, "special values")
    assert want["counts"][1] == 0 and want["filtered"].tolist() == [1, 1, 1] and 0 < want["counts"][0] < N
    for t in out.values():
        t.zero_()      # the NaNs do not go back to the allocator
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
    for enable in (True, False):
        e = ops.query_prefilter(z(2, 0, 2), z(2, 0), z(2, 0, D), z(2, 0, n_class), z(2, 0, dt=torch.int32), z(2, 0, dt=torch.int32), z(2, dt=torch.int32),
                                z(2, dt=torch.int32), enable)
        assert e["counts"].tolist() == [0, 0] and e["filtered"].tolist() == [int(enable)] * 2 and tuple(e["kept"].shape) == (2, 0)


def test_prefilter_entry_statuses(hip_lib, dev):
    """Every error status through the C entry; batch == 0 and n == 0 succeed and write nothing."""
    L = hip_lib
    B, N, n_class = 2, 6, 5
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
    a = {"kp": z(B, N, 2), "sc": z(B, N), "de": z(B, N, 8) + 1, "lo": z(B, N, n_class), "ids": z(B, N, dt=torch.int32), "mask": torch.ones(B, N, device=dev, dtype=torch.int32),
         "nnb": torch.tensor([N, N], device=dev, dtype=torch.int32), "cnt": torch.tensor([N, 2], device=dev, dtype=torch.int32)}
    o = {"kp": z(B, N, 2), "sc": z(B, N), "de": z(B, N + 1, 8), "lo": z(B, N, n_class), "ids": z(B, N, dt=torch.int32), "cnt": torch.full((B,), -7, device=dev, dtype=torch.int32),
         "kept": torch.full((B, N), -7, device=dev, dtype=torch.int32), "fil": torch.full((B,), -7, device=dev, dtype=torch.int32)}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def run(batch=B, n=N, c=n_class, d=8, **kw):
        """keyword k replaces input k, keyword o_k output k"""
        x, y = dict(a), dict(o)
        x.update({k: v for k, v in kw.items() if not k.startswith("o_")})
        y.update({k[2:]: v for k, v in kw.items() if k.startswith("o_")})
        return L.pram_query_prefilter(p(x["kp"]), p(x["sc"]), p(x["de"]), p(x["lo"]), p(x["ids"]), p(x["mask"]), p(x["nnb"]), p(x["cnt"]), 1, batch, n, c, d,
                                      p(y["kp"]), p(y["sc"]), p(y["de"]), p(y["lo"]), p(y["ids"]), p(y["cnt"]), p(y["kept"]), p(y["fil"]), st)
    assert run() == 0
    torch.cuda.synchronize()
    assert o["cnt"].tolist() == [N, 2] and o["fil"].tolist() == [1, 1] and o["kept"][1].tolist() == [0, 1, -1, -1, -1, -1]
    assert o["de"].view(-1)[:B * N * 8].view(B, N, 8)[1].sum().item() == 16 and o["ids"][1].tolist() == [0, 0, -2, -2, -2, -2]
    E_ARG = -1
    for k in a:
        assert run(**{k: None}) == E_ARG and b"null" in L.pram_last_error(), k
    for k in o:
        assert run(**{"o_" + k: None}) == E_ARG and b"null" in L.pram_last_error(), k
    assert run(batch=-1) == E_ARG and b"batch >= 0" in L.pram_last_error()
    assert run(n=-1) == E_ARG and b"n >= 0" in L.pram_last_error()
    assert run(c=0) == E_ARG and b"n_class >= 1" in L.pram_last_error()
    for d in (2, 7, -4):
        assert run(d=d) == E_ARG and b"multiple of 4" in L.pram_last_error(), d
    assert run(de=a["de"].view(-1)[1:]) == E_ARG and b"16-byte" in L.pram_last_error()
    assert run(o_de=o["de"].view(-1)[2:]) == E_ARG and b"16-byte" in L.pram_last_error()
    assert run(lo=a["lo"].view(torch.int8).view(-1)[1:]) == E_ARG and b"misaligned" in L.pram_last_error()
    assert run(o_kp=a["kp"]) == E_ARG and b"must not be the inputs" in L.pram_last_error()
    for k in ("cnt", "kept", "fil"):
        o[k].fill_(-7)
    assert run(batch=0) == 0 and run(n=0) == 0
    torch.cuda.synchronize()
    assert o["cnt"].tolist() == [-7, -7] and o["fil"].tolist() == [-7, -7] and (o["kept"] == -7).all()


# ---------------------------------------------------------------- the pinned cases through prefilter_queries
def test_pinned_cases_through_prefilter_queries(dev, golden):
    """prefilter_pinned.npz and the three segpost_* goldens, batched together per threshold: kept and seg_ids equal the
    reference's; the dict form with the recogniser epilogue's outputs gives the same as the plain prediction."""
    from pram_amd import ops
    from pram_amd.localization.localizer import prefilter_queries
    g = golden("prefilter_pinned")
    seg_logits = golden("segpost_logits")["logits"]
    rng = np.random.default_rng(3)
    for th, tag in ((0.95, "thr095"), (0.2, "thr02"), (0.0, "thr0")):
        s = golden(f"segpost_{tag}")
        cases = [(g[f"case{i}_logits"], g[f"case{i}_kept"], g[f"case{i}_seg_ids"]) for i in range(int(g["n_cases"])) if float(g[f"case{i}_threshold"]) == th]
        # the segpost logits have 113 classes, the pinned cases 29: the narrower rows are widened with classes that never win
        cases = [(np.concatenate([l, np.full((len(l), seg_logits.shape[1] - l.shape[1]), -60.0, np.float32)], 1), k, i) for l, k, i in cases]
        cases.append((seg_logits, s["kept"], s["seg_ids"]))
        B, N, Cc = len(cases), 400, seg_logits.shape[1]
        counts = np.array([len(c[0]) for c in cases], dtype=np.int32)
        logits = rng.standard_normal((B, N, Cc)).astype(np.float32)
        for b, c in enumerate(cases):
            logits[b, :counts[b]] = c[0]
        feats = {"keypoints": torch.from_numpy(rng.standard_normal((B, N, 2)).astype(np.float32)).to(dev), "scores": torch.rand(B, N, device=dev),
                 "descriptors": torch.randn(B, N, D, device=dev), "counts": torch.from_numpy(counts).to(dev), "image_size": (640, 480)}
        pred = torch.from_numpy(logits).to(dev)
        f1, r1, info = prefilter_queries(feats, pred, th)
        ids, mask, cnt, _ = ops.seg_epilogue(pred, feats["counts"], th if th > 0 else 2.0)
        f2, r2, info2 = prefilter_queries(feats, {"prediction": pred, "landmark": ids, "non_bg": mask, "n_non_bg": cnt, "bg_threshold": th}, th)
        stale = {"prediction": pred, "landmark": ids, "non_bg": torch.ones_like(mask), "n_non_bg": feats["counts"], "bg_threshold": 0.5}      # another threshold's: not reused
        f3, r3, info3 = prefilter_queries(feats, stale, th)
        assert f1["image_size"] == (640, 480) and set(r1) == {"prediction", "seg_ids"} and set(info) == {"kept", "filtered", "counts_before"}
        assert torch.equal(info["counts_before"], feats["counts"]) and all(v.is_cuda for v in info.values())
        for (fa, ra, ia) in ((f2, r2, info2),) + (((f3, r3, info3),) if th > 0 else ()):
            for k in ("keypoints", "scores", "descriptors", "counts"):
                assert torch.equal(f1[k], fa[k]), k
            assert torch.equal(r1["prediction"], ra["prediction"]) and torch.equal(r1["seg_ids"], ra["seg_ids"]) and torch.equal(info["kept"], ia["kept"])
        kept, seg_ids, n_out = info["kept"].cpu().numpy(), r1["seg_ids"].cpu().numpy(), f1["counts"].cpu().numpy()
        for b, (l, k, i) in enumerate(cases):
            m = len(k)
            assert n_out[b] == m and np.array_equal(kept[b, :m], k) and (kept[b, m:] == -1).all(), (tag, b)
            assert np.array_equal(seg_ids[b, :m], i) and (seg_ids[b, m:] == -2).all(), (tag, b)
            assert torch.equal(f1["descriptors"][b, :m], feats["descriptors"][b][torch.from_numpy(k).long().to(dev)])
        assert n_out[-1] == {"thr095": 396, "thr02": 235, "thr0": 400}[tag]
        want = LR.prefilter_batch({"keypoints": feats["keypoints"].cpu().numpy(), "scores": feats["scores"].cpu().numpy(), "descriptors": feats["descriptors"].cpu().numpy(),
                                   "logits": logits}, counts, th)
        for k in ("keypoints", "scores", "descriptors"):
            assert np.array_equal(_bits(f1[k]), _bits(want[k])), k
        assert np.array_equal(_bits(r1["prediction"]), _bits(want["logits"])) and np.array_equal(info["filtered"].cpu().numpy(), want["filtered"])


# ---------------------------------------------------------------- run_features on the seeded sequence
LOC = dict(seg_k=RR.SEG_K, min_kpts=32, threshold=4.0, min_inliers=20, semantic_matching=False, trials=1000, seed=4)
REFINE_BELOW, N_MAX, TH = 80, 256, 0.95      # tests/test_gpu_track.py's arguments
EXTRA_BASE, EXTRA_CLUTTER = 1, 110           # the fifth query: stream 1's frame plus 110 clutter rows, so under 40 % are off the background


def _gml(dev, precision=None):
    from pram_amd.nets.gml import GML
    g = GML({})
    g.load_state_dict(H.gml_sd(), strict=True)
    g.precision = precision
    return g.to(dev).eval()


def _cluttered(q: dict, seed: int) -> dict:
    """A scene query with EXTRA_CLUTTER more clutter rows (random unit descriptors, random positions, logits peaking on the
    background), interleaved with its own rows by a seeded permutation."""
    rng = np.random.default_rng(seed)
    n0, w, h = q["count"], q["width"], q["height"]
    n = n0 + EXTRA_CLUTTER
    assert n <= RR.N_PAD
    seg = rng.standard_normal((EXTRA_CLUTTER, RR.N_CLASS)).astype(np.float32)
    seg[:, 0] += 10.0
    rows = {"keypoints": np.concatenate([q["keypoints"], np.stack([rng.uniform(4, w - 4, EXTRA_CLUTTER), rng.uniform(4, h - 4, EXTRA_CLUTTER)], 1).astype(np.float32)]),
            "scores": np.concatenate([q["scores"], rng.uniform(0, 1, EXTRA_CLUTTER).astype(np.float32)]),
            "descriptors": np.concatenate([q["descriptors"], CR._unit(rng.standard_normal((EXTRA_CLUTTER, 128))).astype(np.float32)]),
            "segmentations": np.concatenate([q["segmentations"], seg])}
    perm = rng.permutation(n)
    out = {k: v[perm] for k, v in rows.items()}
    out.update(width=w, height=h, count=n, seg_ids=(np.argmax(out["segmentations"], 1) - 1).astype(np.int32))
    out["padded"] = {k: np.concatenate([out[k], np.zeros((RR.N_PAD - n,) + out[k].shape[1:], dtype=out[k].dtype)]) for k in rows}
    return out


@pytest.fixture(scope="module")
def scene(dev):
    from pram_amd.localization.candidates import ReferenceStore
    m, frames, planted = TR.sequence_scene()
    store = ReferenceStore(m["frames"], m["seg_ref_frame_ids"], m["start_sid"], device=dev, covisibility_frame=RR.COVIS)
    steps, hand, cams, filtered = [], [], [], []
    for t in range(TR.N_FRAMES):
        qs = list(frames[t]) + [_cluttered(frames[t][EXTRA_BASE], 50 + t)]
        feats, seg = CR.batch_features(qs, dev)
        counts = np.array([q["count"] for q in qs])
        arrays = {k: np.stack([q["padded"][k] for q in qs]) for k in ("keypoints", "scores", "descriptors")}
        arrays["logits"] = np.stack([q["padded"]["segmentations"] for q in qs])
        for b, q in enumerate(qs):      # no row's background probability stands near the threshold
            if q["count"]:
                assert np.abs(LR.softmax64(q["segmentations"])[:, 0] - TH).min() >= 1e-4, (t, b)
        want = LR.prefilter_batch(arrays, counts, TH)
        steps.append((feats, seg))
        hand.append(want)
        cams.append([p["cam"] for p in planted[t]] + [planted[t][EXTRA_BASE]["cam"]])
        filtered.append(want["filtered"].tolist())
    return {"map": m, "frames": frames, "planted": planted, "store": store, "steps": steps, "hand": hand, "cams": cams, "filtered": filtered}


def _hand_inputs(want, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    feats = {"keypoints": t(want["keypoints"]), "scores": t(want["scores"]), "descriptors": t(want["descriptors"]), "counts": t(want["counts"]),
             "image_size": RR.CAMERA}
    return feats, t(want["logits"])


def _same_result(got, want, what):
    assert got["success"] == want["success"] and got.get("source") == want.get("source"), what
    assert got["reference_frame_id"] == want["reference_frame_id"] and got["num_inliers"] == want["num_inliers"], what
    if not want["success"]:
        return
    assert np.array_equal(got["qvec"], want["qvec"]) and np.array_equal(got["tvec"], want["tvec"]), what      # bit-equal poses
    assert torch.equal(got["inliers"], want["inliers"]), what
    for k in TR.LIST_KEYS:
        assert (got.get(k) is None) == (want.get(k) is None), (what, k)
        if want.get(k) is not None:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)


def _run_scene(scene, dev, precision, method, tracking):
    from pram_amd.localization.localizer import Localizer, pose_errors
    from pram_amd.localization.refine import localize_and_refine
    from pram_amd.localization.tracker import Tracker
    from pram_amd.pipeline import QueryPipeline
    net = _gml(dev, precision)
    B = TR.N_STREAMS + 1
    kw = dict(LOC, refine_below=REFINE_BELOW, refinement_method=method, covisibility_frame=RR.COVIS)
    loc = Localizer(QueryPipeline(None, None, net), scene["store"], pre_filtering_th=TH, tracking=tracking, n_streams=B, n_max=N_MAX, **kw)
    hand = Tracker(scene["store"], net, B, N_MAX, **kw) if tracking else None
    seen = {"fired": 0, "not_fired": 0, "empty": 0, "tracked": 0, "located": 0}
    for t in range(TR.N_FRAMES):
        feats, seg = scene["steps"][t]
        want_arrays, cams = scene["hand"][t], scene["cams"][t]
        res = loc.run_features(feats, seg, cams)
        hf, hp = _hand_inputs(want_arrays, dev)
        if tracking:
            want = hand.run(hf, hp, cams)
            assert loc.tracker.lost.tolist() == hand.lost.tolist()
            for k in hand.state.FIELDS:
                assert torch.equal(getattr(loc.tracker.state, k), getattr(hand.state, k)), (t, k)
        else:
            ref_kw = {k: v for k, v in kw.items() if k != "refine_below"}
            want = localize_and_refine(hf, hp, scene["store"], net, cams, **ref_kw)
        assert len(res) == len(want) == B
        for b in range(B):
            what = f"[{precision} {method} tracking={tracking}] step {t} query {b}"
            r = res[b]
            _same_result(r, want[b], what)
            n_before, n_after = int(feats["counts"][b]), int(want_arrays["counts"][b])
            assert r["n_keypoints"] == (n_before, n_after), what
            assert r["kept"].is_cuda and np.array_equal(r["kept"].cpu().numpy(), want_arrays["kept"][b, :n_after]), what
            fired = bool(want_arrays["filtered"][b])
            seen["empty"] += n_before == 0
            seen["fired"] += fired and n_before > 0
            seen["not_fired"] += (not fired) and n_before > 0
            if fired and n_before:      # the filter lost none of the frame's map points
                q = (list(scene["frames"][t]) + [None])[b]
                if q is not None:
                    assert n_after < n_before and set(np.nonzero(q["pool"] >= 0)[0].tolist()) <= set(want_arrays["kept"][b, :n_after].tolist()), what
            if not r["success"]:
                continue
            seen["located"] += 1
            # kept[matched_keypoint_ids] names the rows of the unfiltered frame that hold the same keypoints
            rows = r["kept"][r["matched_keypoint_ids"]].long()
            assert torch.equal(feats["keypoints"][b][rows], r["matched_keypoints"]), what
            if tracking and r["source"] in ("track", "track+refine") and len(r["matched_keypoint_ids"]) >= 64 and b < TR.N_STREAMS:
                p = scene["planted"][t][b]
                er, ec = pose_errors([r["qvec"]], [r["tvec"]], [PR.rot_to_qvec(p["R"])], [p["t"]])
                print(f"localizer {what} {r['source']}: {er[0]:.4f} deg, {ec[0]:.4f} m from the planted camera, {r['num_inliers']}/{len(r['matched_keypoint_ids'])} inliers")
                assert er[0] < 1.0 and ec[0] < 0.5, what
                seen["tracked"] += 1
        print(f"localizer [{precision} {method} tracking={tracking}] step {t}: {[r.get('source', r['success']) for r in res]} n_keypoints {[r['n_keypoints'] for r in res]}")
    # both branches of the filter and the empty stream went through the whole chain
    assert seen["fired"] >= 3 * TR.N_FRAMES and seen["not_fired"] >= TR.N_FRAMES and seen["empty"] >= TR.N_FRAMES and seen["located"] >= 3
    if tracking:
        assert seen["tracked"] >= 1
    return loc


@pytest.mark.parametrize("tracking", [True, False])
@pytest.mark.parametrize("precision,method", [("x3", "matching"), ("f32", "projection"), ("x3", "projection"), ("f32", "matching")])
def test_run_features_equals_the_stages_by_hand(scene, dev, precision, method, tracking):
    """Three frames of sequence_scene plus a cluttered fifth query, pre_filtering_th = 0.95: every result equals Tracker.run (or
    localize_and_refine) called by hand on the restatement's filtered arrays — lists as bits, source, lost, reference_frame_id,
    bit-equal poses, the tracker's whole state; kept / n_keypoints equal the restatement's; kept[matched_keypoint_ids] names the
    extractor's rows; a tracked query with 64 matches or more stands within 1 degree / 0.5 m of its planted camera."""
    assert [f[:3] for f in scene["filtered"]] == [[1, 1, 1]] * TR.N_FRAMES and all(f[4] == 0 for f in scene["filtered"])
    loc = _run_scene(scene, dev, precision, method, tracking)
    if tracking:
        loc.reset([0])
        assert loc.tracker.lost[0] and not loc.tracker.lost[1]
        loc.reset()
        assert loc.tracker.lost.all()


def test_run_features_without_refinement_and_without_filter(scene, dev):
    """do_refinement = False goes to localize_candidates; pre_filtering_th = 0 hands the frames on as they are (kept = arange)."""
    from pram_amd.localization.localizer import Localizer
    from pram_amd.localization.pose import localize_candidates
    from pram_amd.pipeline import QueryPipeline
    net = _gml(dev)
    feats, seg = scene["steps"][0]
    cams = scene["cams"][0]
    loc = Localizer(QueryPipeline(None, None, net), scene["store"], pre_filtering_th=0.0, do_refinement=False, **LOC)
    res = loc.run_features(feats, {"prediction": seg}, cams)
    want = localize_candidates(feats, seg, scene["store"], net, cams, **LOC)
    for b, (r, w) in enumerate(zip(res, want)):
        _same_result(r, w, f"no filter, query {b}")
        n = int(feats["counts"][b])
        assert r["n_keypoints"] == (n, n) and r["kept"].tolist() == list(range(n)) and "refinement" not in r


@pytest.mark.parametrize("tracking", [True, False])
def test_cameras_resident_on_the_device(scene, dev, tracking):
    """device_cameras' result carries no image size, which the projection refinement needs: the Localizer hands it the batch's.
    Two frames under refinement_method = 'projection' equal the same frames with camera tuples (all 640 x 480, the batch's size)."""
    from pram_amd.localization.localizer import Localizer
    from pram_amd.localization.pose import device_cameras
    from pram_amd.pipeline import QueryPipeline
    net = _gml(dev)
    kw = dict(LOC, refine_below=REFINE_BELOW, refinement_method="projection", covisibility_frame=RR.COVIS)
    a, b = (Localizer(QueryPipeline(None, None, net), scene["store"], pre_filtering_th=TH, tracking=tracking, n_max=N_MAX, **kw) for _ in range(2))
    refined = 0
    for t in range(2):
        feats, seg = scene["steps"][t]
        cams = scene["cams"][t]
        assert all(c[1:3] == feats["image_size"] for c in cams)
        ra, rb = a.run_features(feats, seg, cams), b.run_features(feats, seg, device_cameras(cams, dev))
        for q, (x, y) in enumerate(zip(ra, rb)):
            _same_result(x, y, f"device cameras, tracking={tracking}, step {t} query {q}")
            for r in (x.get("tracking"), x.get("localization"), x):
                refined += bool(r) and (r.get("refinement") or {}).get("method") == "projection"
    assert refined >= 1


# ---------------------------------------------------------------- run from images
def test_run_from_images_equals_the_stages_by_hand(scene, dev):
    """Two 480 x 640 frames through the nets of tests/helpers.py's state dicts: Localizer.run equals pipeline.run(..., 'er'), then
    prefilter_queries, then Tracker.run, called by hand — with the pipeline's own epilogue reused (the same threshold) and with
    another threshold (the epilogue runs again).  Random weights: no pose is expected; the assertion is the equality and the shapes."""
    from pram_amd import weights as W
    from pram_amd.localization.localizer import Localizer, prefilter_queries
    from pram_amd.localization.tracker import Tracker
    from pram_amd.nets.load_segnet import load_segnet
    from pram_amd.nets.sfd2 import ResNet4x
    from pram_amd.pipeline import QueryPipeline
    sfd2, seg, gml = ResNet4x(), load_segnet('segnetvit', 113, 256, 15, 1024), _gml(dev)
    for m, sd in ((sfd2, H.sfd2_sd()), (seg, H.segnet_sd(113))):
        m.load_state_dict(sd, strict=True)
        m.to(dev).eval()
    k = 192
    pipe = QueryPipeline(sfd2, seg, gml, max_keypoints=k, min_keypoints=8)
    images = torch.stack([W.synthetic_image(1, 480, 640), W.synthetic_image(4, 480, 640) * 0.3]).to(dev)
    cams = [("PINHOLE", 640, 480, [520.0, 520.0, 320.0, 240.0])] * 2
    kw = dict(LOC, refine_below=REFINE_BELOW, covisibility_frame=RR.COVIS)
    for th in (pipe.bg_threshold, 0.5):
        loc = Localizer(pipe, scene["store"], pre_filtering_th=th, tracking=True, **kw)
        res = loc.run(images, cams)
        assert loc.tracker.n_streams == 2 and loc.tracker.n_max == k
        out = pipe.run(images, None, stages="er")
        feats = {key: out[key] for key in ("keypoints", "scores", "descriptors", "counts")}
        feats["image_size"] = (640, 480)
        f, r, info = prefilter_queries(feats, out["prediction"], th)
        want = Tracker(scene["store"], gml, 2, k, **kw).run(f, r, cams)
        n_before, n_after, kept = out["counts"].tolist(), f["counts"].tolist(), info["kept"]
        assert len(res) == 2
        for b in range(2):
            _same_result(res[b], want[b], f"images th={th} query {b}")
            assert res[b]["n_keypoints"] == (n_before[b], n_after[b]) and 0 < n_after[b] <= n_before[b] <= k
            assert tuple(res[b]["kept"].shape) == (n_after[b],) and torch.equal(res[b]["kept"], kept[b, :n_after[b]])
        print(f"localizer from images th={th}: n_keypoints {[x['n_keypoints'] for x in res]}, filtered {info['filtered'].tolist()}, success {[x['success'] for x in res]}")


# ---------------------------------------------------------------- the evaluation helpers
def test_pose_errors_and_recall_on_the_planted_cameras(scene):
    """pose_errors between the planted cameras of consecutive frames (a stream moves about 0.2 degrees and 5 cm per frame; stream
    2 jumps) against the restatement (1e-12) and against pose_ref.pose_errors, which takes the angle from the rotation matrices'
    trace (both forms lose at most eps / angle radians: 1e-6 degrees and 1e-9 m are far above that)."""
    from pram_amd.localization.localizer import pose_errors, recall_counts
    pl = scene["planted"]
    pairs = [(pl[t][s], pl[t + 1][s]) for t in range(TR.N_FRAMES - 1) for s in range(TR.N_STREAMS)]
    qs, ts = [PR.rot_to_qvec(a["R"]) for a, _ in pairs] + [None], [a["t"] for a, _ in pairs] + [None]
    gqs, gts = [PR.rot_to_qvec(b["R"]) for _, b in pairs] + [qs[0]], [b["t"] for _, b in pairs] + [ts[0]]
    q_err, t_err = pose_errors(qs, ts, gqs, gts)
    rq, rt = LR.pose_errors(qs, ts, gqs, gts)
    assert np.abs(q_err - rq).max() <= 1e-12 and np.abs(t_err - rt).max() <= 1e-12
    for i, (a, b) in enumerate(pairs):
        er, ec = PR.pose_errors(a["R"], a["t"], b["R"], b["t"])
        assert abs(q_err[i] - er) <= 1e-6 and abs(t_err[i] - ec) <= 1e-9, (i, q_err[i], er, t_err[i], ec)
    assert q_err[-1] == 100 and t_err[-1] == 100
    cnt = recall_counts(q_err, t_err)
    assert cnt.tolist() == LR.recall_counts(q_err, t_err).tolist() and cnt[3] >= cnt[2] >= cnt[0] and cnt[3] <= len(pairs)
    print(f"localizer: errors between consecutive planted cameras: {np.round(q_err, 3).tolist()} deg, {np.round(t_err, 3).tolist()} m, recall {cnt.tolist()}")
