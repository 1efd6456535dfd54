"""Numpy restatement of the reference's query pre-filter and pose evaluation, for the tests of pram_amd.localization.localizer.

Written from Frame.add_segmentations (localization/frame.py:96-121), Frame.compute_pose_error (frame.py:139-152),
localization/utils.py:26-53 and the counters of localization/loc_by_rec_eval.py:272-279.  Plain host loops over plain numpy, one
query at a time; the batch form only pads what the one-frame form returns."""
from __future__ import annotations

import numpy as np

ROW_KEYS = ("keypoints", "scores", "descriptors", "logits", "seg_ids")
SEG_FILL = -2      # pram_seg_epilogue_f32's fill of seg_ids beyond the count


def softmax64(logits) -> np.ndarray:
    """torch.softmax(dim=-1) in float64: exp(x - max) / sum"""
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True)) if x.shape[-1] else x
    return e / e.sum(axis=-1, keepdims=True)


def non_bg_mask(logits, threshold: float) -> np.ndarray:
    """frame.py:103-104 on one frame's logits [n, C] -> bool [n].  (float64: the fixtures keep every background probability away
    from its threshold, so the float32 softmax of the reference decides the same.)"""
    logits = np.asarray(logits)
    if logits.shape[0] == 0:
        return np.zeros(0, dtype=bool)
    return softmax64(logits)[:, 0] < threshold


def fires(n_non_bg: int, n: int, threshold: float) -> bool:
    """frame.py:102, 106: the right side is a Python float product"""
    return threshold > 0 and int(n_non_bg) >= 0.4 * int(n)


def add_segmentations(logits, threshold: float, mask=None, n_non_bg=None):
    """One frame: logits [n, C] -> (kept int64 [m]: the rows the frame keeps, in order; seg_ids int32 [m] = argmax - 1 of the kept
    rows; filtered: whether the filter fired).  mask: the non-background mask to use (None: computed here); n_non_bg: the count
    the decision is taken on (None: the mask's own sum, as in the reference; the device entry is handed the recogniser
    epilogue's count, and its tests hand it others)."""
    logits = np.asarray(logits)
    n = logits.shape[0]
    kept, filtered = np.arange(n, dtype=np.int64), False
    if threshold > 0:
        m = non_bg_mask(logits, threshold) if mask is None else np.asarray(mask).astype(bool)[:n]
        if fires(int(m.sum()) if n_non_bg is None else int(n_non_bg), n, threshold):
            kept, filtered = np.nonzero(m)[0].astype(np.int64), True
    seg = logits[kept]
    seg_ids = (np.argmax(seg, axis=1) - 1).astype(np.int32) if len(kept) else np.zeros(0, np.int32)
    return kept, seg_ids, filtered


def prefilter_batch(arrays: dict, counts, threshold: float, masks=None, seg_ids=None, n_non_bg=None) -> dict:
    """The padded batch.  arrays: keypoints [B, N, 2], scores [B, N], descriptors [B, N, D], logits [B, N, C] (any dtype; rows are
    moved, never computed on); counts [B]; masks [B, N]: the non-background masks to use (None: computed from the logits);
    seg_ids [B, N]: the labels to move (None: argmax - 1); n_non_bg [B]: the counts the decisions are taken on (None: the masks'
    sums).  -> the five row arrays compacted (zero beyond the new count, seg_ids -2 there), counts, kept int32 [B, N] (-1 beyond
    the new count), filtered int32 [B], counts_before."""
    counts = np.asarray(counts).astype(np.int64)
    B, N = np.asarray(arrays["scores"]).shape
    out = {k: np.zeros_like(np.asarray(arrays[k])) for k in ROW_KEYS if k != "seg_ids"}
    out["seg_ids"] = np.full((B, N), SEG_FILL, dtype=np.int32)
    out["kept"], out["counts"] = np.full((B, N), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    out["filtered"], out["counts_before"] = np.zeros(B, dtype=np.int32), counts.astype(np.int32)
    for b in range(B):
        n = int(min(max(counts[b], 0), N))
        logits = np.asarray(arrays["logits"])[b, :n]
        kept, ids, f = add_segmentations(logits, threshold, None if masks is None else np.asarray(masks)[b, :n],
                                         None if n_non_bg is None else np.asarray(n_non_bg)[b])
        m = len(kept)
        for k in ("keypoints", "scores", "descriptors", "logits"):
            out[k][b, :m] = np.asarray(arrays[k])[b, kept]
        out["seg_ids"][b, :m] = ids if seg_ids is None else np.asarray(seg_ids)[b, kept]
        out["kept"][b, :m], out["counts"][b], out["filtered"][b] = kept, m, int(f)
    return out


# ---------------------------------------------------------------- evaluation
def rotation(qvec) -> np.ndarray:
    """(w, x, y, z) -> the rotation matrix, float64"""
    w, x, y, z = (float(v) for v in qvec)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def pose_error(qvec, tvec, gt_qvec, gt_tvec):
    """utils.py:26-53 for one query; frame.py:139-152: (100, 100) without a pose."""
    if qvec is None or tvec is None or gt_qvec is None or gt_tvec is None:
        return 100.0, 100.0
    c = -rotation(qvec).T @ np.asarray(tvec, dtype=np.float64).reshape(3, 1)
    gc = -rotation(gt_qvec).T @ np.asarray(gt_tvec, dtype=np.float64).reshape(3, 1)
    t_err = float(np.sqrt(np.sum((c - gc) ** 2)))
    d = abs(float(np.dot(np.asarray(qvec, dtype=np.float64), np.asarray(gt_qvec, dtype=np.float64))))
    d = min(1.0, max(-1.0, d))
    return float(2 * np.arccos(d) * 180 / np.pi), t_err


def pose_errors(qvecs, tvecs, gt_qvecs, gt_tvecs):
    e = [pose_error(q, t, gq, gt) for q, t, gq, gt in zip(qvecs, tvecs, gt_qvecs, gt_tvecs)]
    return np.array([x[0] for x in e], dtype=np.float64), np.array([x[1] for x in e], dtype=np.float64)


def recall_counts(q_err, t_err) -> np.ndarray:
    """loc_by_rec_eval.py:272-279"""
    cnt = np.zeros(4, dtype=np.int64)
    for q, t in zip(q_err, t_err):
        cnt[0] += q <= 5 and t <= 0.05
        cnt[1] += q <= 2 and t <= 0.25
        cnt[2] += q <= 5 and t <= 0.5
        cnt[3] += q <= 10 and t <= 5
    return cnt


# ---------------------------------------------------------------- the cases pinned by running the reference
PINNED_SEED, PINNED_CLASSES, PINNED_MARGIN = 11, 29, 1e-4
PINNED_SIZES = (0, 1, 5, 63, 64, 65, 257, 400)
PINNED_THRESHOLDS = (0.0, 0.2, 0.95)


def _logits_with_share(rng, n: int, n_non_bg: int, threshold: float, n_class: int = PINNED_CLASSES) -> np.ndarray:
    """n rows of which exactly n_non_bg (seeded positions) have a background probability below the threshold, every row at least
    PINNED_MARGIN away from it: the background logit is moved until the row stands clear on its side."""
    x = rng.standard_normal((n, n_class)).astype(np.float32) * 2.0
    non_bg = np.zeros(n, dtype=bool)
    non_bg[rng.permutation(n)[:n_non_bg]] = True
    th = threshold if threshold > 0 else 0.5
    for i in range(n):
        for _ in range(200):
            p = softmax64(x[i])[0]
            if (p < th - 10 * PINNED_MARGIN) if non_bg[i] else (p > th + 10 * PINNED_MARGIN):
                break
            x[i, 0] += np.float32(-0.37 if non_bg[i] else 0.37)
        else:
            raise AssertionError("no background logit puts the row clear of the threshold")
    return x


def pinned_cases(seed: int = PINNED_SEED):
    """The inputs of tests/tools/gen_prefilter_pinned.py, rebuilt from the seed: every size x every threshold with a seeded share
    of non-background rows on either side of 40 %, plus n = 5 with exactly 2 non-background rows (fires: 2 >= 2.0) and n = 5 with
    exactly 1 (does not).  -> list of dict(n, threshold, logits [n, C] float32)."""
    rng = np.random.default_rng(seed)
    cases = []
    for n in PINNED_SIZES:
        for th in PINNED_THRESHOLDS:
            share = (0.25, 0.7)[len(cases) % 2]
            cases.append({"n": n, "threshold": th, "logits": _logits_with_share(rng, n, int(round(share * n)), th)})
    for k, th in ((2, 0.95), (1, 0.95), (2, 0.2), (1, 0.2)):
        cases.append({"n": 5, "threshold": th, "logits": _logits_with_share(rng, 5, k, th)})
    return cases


def pinned_poses(seed: int = PINNED_SEED):
    """Pose pairs for the evaluation helpers: errors on both sides of every recall bar, an exact copy (|q . q_gt| rounds above 1),
    a sign-flipped quaternion, and queries without a pose.  -> (qvecs, tvecs, gt_qvecs, gt_tvecs), lists with None entries."""
    rng = np.random.default_rng(seed + 1)
    qs, ts, gqs, gts = [], [], [], []
    steps = ((0.0, 0.0), (0.5, 0.01), (1.9, 0.04), (1.9, 0.2), (2.5, 0.2), (4.5, 0.045), (4.5, 0.3), (4.9, 0.49), (6.0, 0.3), (9.0, 3.0), (9.5, 6.0), (30.0, 0.01), (0.1, 40.0))
    for i, (deg, dist) in enumerate(steps):
        gq = rng.standard_normal(4)
        gq /= np.linalg.norm(gq)
        gt = rng.standard_normal(3) * 3
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        half = np.deg2rad(deg) / 2
        dq = np.concatenate([[np.cos(half)], np.sin(half) * axis])
        w0, v0, w1, v1 = dq[0], dq[1:], gq[0], gq[1:]
        q = np.concatenate([[w0 * w1 - v0 @ v1], w0 * v1 + w1 * v0 + np.cross(v0, v1)])
        shift = rng.standard_normal(3)
        shift *= dist / np.linalg.norm(shift)
        c = -rotation(gq).T @ gt + shift
        t = -rotation(q) @ c
        if i % 4 == 3:
            q = -q
        qs.append(q), ts.append(t), gqs.append(gq), gts.append(gt)
    qs.append(None), ts.append(None), gqs.append(gqs[0]), gts.append(gts[0])
    qs.append(qs[1]), ts.append(None), gqs.append(gqs[1]), gts.append(gts[1])
    return qs, ts, gqs, gts
