"""CPU: the numpy restatement tests/localizer_ref.py against the fixtures recorded from the reference (prefilter_pinned.npz, the
segpost_* goldens), the host-side evaluation helpers of pram_amd.localization.localizer against the same pins, the new entry's
export, and the usual error on CPU tensors."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import localizer_ref as LR

ROOT = Path(__file__).resolve().parents[1]
ERR_BAR = 1e-12      # the issue's bar for the errors: bit-equal or within 1e-12


def _cases(g):
    return [{"logits": g[f"case{i}_logits"], "threshold": float(g[f"case{i}_threshold"]), "kept": g[f"case{i}_kept"], "seg_ids": g[f"case{i}_seg_ids"]}
            for i in range(int(g["n_cases"]))]


def test_restatement_reproduces_the_pinned_cases(golden):
    g = golden("prefilter_pinned")
    cases = _cases(g)
    rebuilt = LR.pinned_cases(int(g["seed"]))
    assert len(cases) == len(rebuilt) == 28
    fired = not_fired = 0
    for c, r in zip(cases, rebuilt):
        assert np.array_equal(c["logits"], r["logits"]) and c["threshold"] == r["threshold"]      # the cases regenerate from the seed
        kept, ids, f = LR.add_segmentations(c["logits"], c["threshold"])
        assert np.array_equal(kept, c["kept"]) and np.array_equal(ids, c["seg_ids"]), (r["n"], c["threshold"])
        assert f == (c["threshold"] > 0 and 5 * int(LR.non_bg_mask(c["logits"], c["threshold"]).sum()) >= 2 * r["n"])
        fired, not_fired = fired + f, not_fired + (not f)
        if r["n"] and c["threshold"] > 0:
            assert np.abs(LR.softmax64(c["logits"])[:, 0] - c["threshold"]).min() >= LR.PINNED_MARGIN
    assert sorted({len(c["logits"]) for c in cases}) == sorted(LR.PINNED_SIZES) and {c["threshold"] for c in cases} == set(LR.PINNED_THRESHOLDS)
    # n = 5: exactly two non-background rows fire (2 >= 2.0), exactly one does not
    assert [len(c["kept"]) for c in cases[-4:]] == [2, 5, 2, 5] and all(len(c["logits"]) == 5 for c in cases[-4:])
    assert fired >= 8 and not_fired >= 8


def test_restatement_batched_equals_one_frame_at_a_time(golden):
    cases = _cases(golden("prefilter_pinned"))
    rng = np.random.default_rng(5)
    for th in (0.2, 0.95):
        sel = [c for c in cases if c["threshold"] == th]
        B, N, C = len(sel), 400, LR.PINNED_CLASSES
        arrays = {"keypoints": rng.standard_normal((B, N, 2)).astype(np.float32), "scores": rng.standard_normal((B, N)).astype(np.float32),
                  "descriptors": rng.standard_normal((B, N, 8)).astype(np.float32), "logits": rng.standard_normal((B, N, C)).astype(np.float32) + 9.0}
        counts = np.array([len(c["logits"]) for c in sel])
        for b, c in enumerate(sel):
            arrays["logits"][b, :counts[b]] = c["logits"]
        out = LR.prefilter_batch(arrays, counts, th)
        for b, c in enumerate(sel):
            m = len(c["kept"])
            assert out["counts"][b] == m and np.array_equal(out["kept"][b, :m], c["kept"]) and (out["kept"][b, m:] == -1).all()
            assert np.array_equal(out["seg_ids"][b, :m], c["seg_ids"]) and (out["seg_ids"][b, m:] == LR.SEG_FILL).all()
            for k in ("keypoints", "scores", "descriptors", "logits"):
                assert np.array_equal(out[k][b, :m], arrays[k][b, c["kept"]]) and not out[k][b, m:].any()
            assert out["filtered"][b] == (5 * int(LR.non_bg_mask(c["logits"], th).sum()) >= 2 * counts[b])      # a frame may fire and keep every row


def test_restatement_reproduces_the_segpost_goldens(golden):
    logits = golden("segpost_logits")["logits"]
    for thr, tag, n_kept in ((0.95, "thr095", 396), (0.2, "thr02", 235), (0.0, "thr0", 400)):
        g = golden(f"segpost_{tag}")
        kept, ids, f = LR.add_segmentations(logits, thr)
        assert len(kept) == n_kept and np.array_equal(kept, g["kept"]) and np.array_equal(ids, g["seg_ids"]) and f == (thr > 0)


def test_integer_form_of_the_firing_test():
    """5 k >= 2 n (the kernel's form) against k >= 0.4 * n in float64 (frame.py:106), for every n up to 4100 and every k."""
    for n in range(4101):
        k = np.arange(n + 1, dtype=np.int64)
        assert np.array_equal(k >= 0.4 * n, 5 * k >= 2 * n), n
    for n in (10 ** 6, 2 ** 31 - 1, 2 ** 31 - 3, 5 * (2 ** 28)):      # the edges of what an int holds: the boundary k on both sides
        k0 = (2 * n + 4) // 5
        for k in (k0 - 1, k0, k0 + 1):
            assert (k >= 0.4 * n) == (5 * k >= 2 * n), (n, k)


@pytest.mark.parametrize("impl", ["restatement", "package"])
def test_pose_errors_and_recall_match_the_reference(golden, impl):
    g = golden("prefilter_pinned")
    has = g["pose_has"]
    rows = lambda a: [a[b] if has[b] else None for b in range(len(has))]
    qs, ts = rows(g["pose_qvecs"]), rows(g["pose_tvecs"])
    if impl == "restatement":
        pose_errors, recall_counts = LR.pose_errors, LR.recall_counts
    else:
        from pram_amd.localization.localizer import pose_errors, recall_counts
    q_err, t_err = pose_errors(qs, ts, list(g["pose_gt_qvecs"]), list(g["pose_gt_tvecs"]))
    assert q_err.dtype == np.float64 and t_err.dtype == np.float64 and q_err.shape == has.shape
    print(f"pose_errors [{impl}]: max |dq| {np.abs(q_err - g['pose_q_err']).max():.2e}, max |dt| {np.abs(t_err - g['pose_t_err']).max():.2e}")
    assert np.abs(q_err - g["pose_q_err"]).max() <= ERR_BAR and np.abs(t_err - g["pose_t_err"]).max() <= ERR_BAR
    assert (q_err[~has] == 100).all() and (t_err[~has] == 100).all() and (~has).sum() == 2
    assert q_err[0] == 0.0      # |q . q| rounds to or above 1: clamped, no NaN
    cnt = recall_counts(q_err, t_err)
    assert cnt.tolist() == g["recall"].tolist() == [4, 4, 8, 10]
    # both comparisons are inclusive
    assert recall_counts([5.0, 2.0, 5.0, 10.0], [0.05, 0.25, 0.5, 5.0]).tolist() == [1, 1, 3, 4]
    assert recall_counts([np.nextafter(5.0, 6.0)], [0.05]).tolist() == [0, 0, 0, 1] and recall_counts([], []).tolist() == [0, 0, 0, 0]


def test_pinned_poses_regenerate(golden):
    g = golden("prefilter_pinned")
    qs, ts, gqs, gts = LR.pinned_poses(int(g["seed"]))
    for b in range(len(qs)):
        assert (qs[b] is not None and ts[b] is not None) == bool(g["pose_has"][b])
        if g["pose_has"][b]:
            assert np.array_equal(qs[b], g["pose_qvecs"][b]) and np.array_equal(ts[b], g["pose_tvecs"][b])


def test_entry_is_exported_and_declared():
    from pram_amd import _lib, ops
    assert "pram_query_prefilter" in _lib.exported_symbols() and callable(ops.query_prefilter)
    res, args = _lib._SIGS["pram_query_prefilter"]      # against the declaration, type by type: tests/test_abi_contract_cpu.py
    assert res is _lib.I and len(args) == 22
    assert (ROOT / "pram_amd" / "csrc" / "prefilter.hip").exists()
    from pram_amd.localization import localizer
    for name in ("Localizer", "prefilter_queries", "pose_errors", "recall_counts"):
        assert callable(getattr(localizer, name))


def test_cpu_tensors_raise():
    from pram_amd._lib import PramHipError
    from pram_amd.localization.localizer import Localizer, prefilter_queries
    from pram_amd.pipeline import QueryPipeline
    B, N, C = 2, 8, 5
    feats = {"keypoints": torch.zeros(B, N, 2), "scores": torch.zeros(B, N), "descriptors": torch.zeros(B, N, 128),
             "counts": torch.full((B,), N, dtype=torch.int32), "image_size": (640, 480)}
    seg = torch.zeros(B, N, C)
    with pytest.raises(PramHipError, match="CUDA tensor"):
        prefilter_queries(feats, seg, 0.95)
    with pytest.raises(PramHipError, match="CUDA tensor"):
        prefilter_queries(feats, {"prediction": seg}, 0.0)
    loc = Localizer(QueryPipeline(None, None, None), None, pre_filtering_th=0.95, tracking=True, seg_k=2, min_kpts=8, threshold=4.0, min_inliers=10)
    with pytest.raises(PramHipError, match="CUDA tensor"):
        loc.run_features(feats, seg, [("PINHOLE", 640, 480, [500.0, 500.0, 320.0, 240.0])] * B)
    loc.reset()      # no tracker yet: nothing to forward to
    with pytest.raises(TypeError, match="unknown arguments"):
        Localizer(QueryPipeline(None, None, None), None, pre_filtering_th=0.95, seg_kk=2)
