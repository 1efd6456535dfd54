"""Images in, poses out: the per-frame loop of the reference's loc_by_rec_eval.py / loc_by_rec_online.py as one call per batch.

Reference: the loop bodies loc_by_rec_eval.py:150-221 and loc_by_rec_online.py:150-197 — extract, recognise, Frame.
add_segmentations with the scene's pre_filtering_th (localization/frame.py:96-121), then the tracker / relocalisation switch —
and the evaluation of loc_by_rec_eval.py:270-279 (Frame.compute_pose_error frame.py:139-152, localization/utils.py:26-53).

``prefilter_queries`` is add_segmentations' filtering for a padded batch: a frame whose recogniser leaves at least 40 % of its
keypoints off the background keeps only those, in their order, and every later stage (the vote, the matcher, the pose, the
tracker's state) sees the filtered frame, as in the reference.  It runs on the device (pram_query_prefilter) from the mask
pram_seg_epilogue_f32 computed, and makes no host synchronisation.  ``Localizer`` joins QueryPipeline (stages "er"), the
pre-filter and Tracker.run (tracking) or localize_and_refine / localize_candidates (stateless).  ``pose_errors`` and
``recall_counts`` are host-side numpy: the poses are already on the host after the stages' read-back.

Deviations: one image size per batch, as in QueryPipeline; the gt_seg IoU / precision bookkeeping, the viewer and
the timing prints of the reference's loops are not built; dataset I/O is out of scope; the stages' own deviations
(4.11 to 4.16) carry over unchanged."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import pose as _pose
from pram_amd.localization import refine as _refine
from pram_amd.localization.tracker import TRACKER_KEYS, Tracker, split_options  # noqa: F401  (TRACKER_KEYS: the names loc_kw may carry)

_EPILOGUE_KEYS = ("landmark", "non_bg", "n_non_bg")


@torch.no_grad()
def prefilter_queries(features: dict, recognition, filtering_threshold: float) -> Tuple[dict, dict, dict]:
    """Frame.add_segmentations' filtering (frame.py:102-116) for a batch.  features: as match_candidates takes them (keypoints
    [B, N, 2], scores [B, N], descriptors [B, N, D], counts int32 [B], image_size or image).  recognition: the [B, N, C] prediction,
    or a dict with 'prediction' / 'segmentations'; QueryPipeline's output dict is one, and its 'landmark', 'non_bg' and 'n_non_bg'
    are reused when it says they were computed at this threshold ('bg_threshold' == filtering_threshold; Localizer.run records
    it) — otherwise ops.seg_epilogue runs once.  A threshold <= 0 filters nothing.
    -> (features', recognition', info): features' = the filtered arrays, the new counts, image_size / image unchanged;
    recognition' = {'prediction', 'seg_ids'} of the filtered frames (vote_candidates and Tracker.run take it as it is); info =
    {'kept' int32 [B, N] (the extractor's row of filtered row j, -1 beyond the new count), 'filtered' int32 [B], 'counts_before'
    int32 [B]}, all on the device: nothing is read back."""
    th = float(filtering_threshold)
    counts = features["counts"]
    ops._chk(counts, "counts", torch.int32)
    ids = mask = cnt = None
    if isinstance(recognition, dict):
        pred = recognition["segmentations"] if "segmentations" in recognition else recognition["prediction"]
        same = th <= 0 or recognition.get("bg_threshold") == th
        if same and all(recognition.get(k) is not None for k in _EPILOGUE_KEYS):
            ids, mask, cnt = (recognition[k] for k in _EPILOGUE_KEYS)
    else:
        pred = recognition
    ops._chk(pred, "recognition")
    pred, counts = pred.contiguous(), counts.contiguous()
    if pred.dim() != 3 or pred.shape[0] != counts.numel():
        raise ValueError("recognition: expected [B, N, C] with B = len(counts)")
    if ids is None:
        ids, mask, cnt, _ = ops.seg_epilogue(pred, counts, th if th > 0 else 2.0)
    f = ops.query_prefilter(features["keypoints"].contiguous(), features["scores"].contiguous(), features["descriptors"].contiguous(), pred,
                            ids.contiguous(), mask.contiguous(), cnt.contiguous(), counts, th > 0)
    out = {k: v for k, v in features.items() if k not in ("keypoints", "scores", "descriptors", "counts")}
    out.update(keypoints=f["keypoints"], scores=f["scores"], descriptors=f["descriptors"], counts=f["counts"])
    return out, {"prediction": f["logits"], "seg_ids": f["seg_ids"]}, {"kept": f["kept"], "filtered": f["filtered"], "counts_before": counts}


class Localizer:
    """QueryPipeline -> prefilter_queries -> Tracker.run (tracking) or localize_and_refine / localize_candidates (stateless).

    pipeline: the QueryPipeline whose extractor, recogniser and matcher are used; store: a ReferenceStore or a MultiMapStore;
    pre_filtering_th: the scene's pre_filtering_th (<= 0: no filtering); tracking: keep the last frame of n_streams streams and
    track it (the switch of loc_by_rec_eval.py:211-221, which Tracker.run implements, commit included); n_streams, n_max: the
    tracker's state (None: the first batch's size, and the larger of the pipeline's max_keypoints and the first batch's row
    stride); loc_kw: Tracker's keyword arguments (TRACKER_KEYS).  Without tracking nothing is kept between calls.

    The range guard follows the pipeline's policy (pipeline.guard): ``run`` extracts and recognises under QueryPipeline.run's own
    guarded call, and every matcher call of the later stages checks under the same policy.

    ``run`` / ``run_features`` return, per query, the dict of the stage below (Tracker.run's, localize_and_refine's or
    localize_candidates') unchanged plus 'kept' (device int32 [count after the filter]: the extractor's row of every row of the
    filtered frame, so kept[matched_keypoint_ids] names the extractor's keypoints) and 'n_keypoints' = (before, after).

    Host synchronisations: those of the stages below; the pre-filter adds none.  The two count vectors travel to pinned host
    memory by an asynchronous copy that the stages' own read-back completes."""

    def __init__(self, pipeline, store, *, pre_filtering_th: float, tracking: bool = False, n_streams: Optional[int] = None,
                 n_max: Optional[int] = None, **loc_kw):
        self._groups = split_options(loc_kw, "Localizer")
        self.pipeline, self.store, self.matcher = pipeline, store, pipeline.matcher
        self.pre_filtering_th, self.tracking = float(pre_filtering_th), bool(tracking)
        self.n_streams, self.n_max = n_streams, n_max
        self._loc_kw = dict(loc_kw)
        self.do_refinement = bool(loc_kw.get("do_refinement", True))
        self.tracker: Optional[Tracker] = None

    def _the_tracker(self, B: int, N: int, device) -> Tracker:
        if self.tracker is None:
            n_max = self.n_max if self.n_max is not None else max(int(self.pipeline.cfg["max_keypoints"]), N, 1)
            self.tracker = Tracker(self.store, self.matcher, self.n_streams if self.n_streams is not None else max(B, 1), n_max, device=device,
                                   **self._loc_kw)
        return self.tracker

    def reset(self, streams=None) -> None:
        """Mark the streams (None: all) lost (Tracker.reset)."""
        if self.tracker is not None:
            self.tracker.reset(streams)

    @torch.no_grad()
    def run(self, images: torch.Tensor, cameras, streams=None) -> List[dict]:
        """images [B, 3, H, W] as QueryPipeline.run takes them (one image size per batch); cameras, streams: as Tracker.run's."""
        out = self.pipeline.run(images, None, stages="er")
        features = {k: out[k] for k in ("keypoints", "scores", "descriptors", "counts")}
        features["image_size"] = (int(images.shape[-1]), int(images.shape[-2]))
        return self.run_features(features, dict(out, bg_threshold=float(self.pipeline.bg_threshold)), cameras, streams)

    @torch.no_grad()
    def run_features(self, features: dict, recognition, cameras, streams=None) -> List[dict]:
        """The same from the pre-filter on, for callers with their own extractor: features, recognition as prefilter_queries'."""
        feats, rec, info = prefilter_queries(features, recognition, self.pre_filtering_th)
        B, N, dev = feats["counts"].numel(), feats["keypoints"].shape[1], feats["counts"].device
        # before / after counts: an asynchronous copy, complete once a later stage has read anything back
        both = torch.stack([info["counts_before"], feats["counts"]])
        host = torch.empty((2, B), dtype=torch.int32, pin_memory=True)
        host.copy_(both, non_blocking=True)
        copied = torch.cuda.Event()
        copied.record(torch.cuda.current_stream(dev))
        # cameras already on the device carry no image size for the projection refinement: the batch has one (QueryPipeline's rule)
        sizes = None
        if _pose.camera_form(cameras) == "resident":
            w, h = feats["image_size"] if "image_size" in feats else (feats["image"].shape[-1], feats["image"].shape[-2])
            sizes = np.tile(np.array([[int(w), int(h)]], dtype=np.int32), (B, 1))
        with ops.guard_scope(self.pipeline.guard):
            if self.tracking:
                res = self._the_tracker(B, N, dev).run(feats, rec, cameras, streams, image_sizes=sizes)
            else:
                g = self._groups
                if self.do_refinement:
                    res = _refine.localize_and_refine(feats, rec, self.store, self.matcher, cameras, image_sizes=sizes, **g["localize"], **g["pose"], **g["refine"])
                else:
                    res = _pose.localize_candidates(feats, rec, self.store, self.matcher, cameras, **g["localize"], **g["pose"])
        copied.synchronize()      # returns at once after any read-back of the stage; waits only when the stage made none
        n = host.numpy()
        for b, r in enumerate(res):
            r["kept"], r["n_keypoints"] = info["kept"][b, :int(n[1, b])], (int(n[0, b]), int(n[1, b]))
        return res


def _rotations(q: np.ndarray) -> np.ndarray:
    """unit quaternions (w, x, y, z) [B, 4] -> rotation matrices [B, 3, 3], float64"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y], -1),
                     np.stack([2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x], -1),
                     np.stack([2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2], -1)], 1)


NOT_LOCATED_ERROR = 100.0      # frame.py:139-152: a frame without a pose reports (100, 100)


def pose_errors(qvecs, tvecs, gt_qvecs, gt_tvecs) -> Tuple[np.ndarray, np.ndarray]:
    """localization/utils.py:26-53 for a batch, float64 on the host.  qvecs [B] of (w, x, y, z) and tvecs [B] of 3 (world to
    camera); an entry that is None (a query that was not located: what the stages report) gives (100, 100), as Frame.
    compute_pose_error does (frame.py:139-152).  -> (q_err_deg [B] = 2 arccos(min(1, |q . q_gt|)) in degrees, t_err [B] = the
    distance between the camera centres -R^T t)."""
    B = len(qvecs)
    q_err, t_err = np.full(B, NOT_LOCATED_ERROR), np.full(B, NOT_LOCATED_ERROR)
    ok = np.array([qvecs[b] is not None and tvecs[b] is not None and gt_qvecs[b] is not None and gt_tvecs[b] is not None for b in range(B)], dtype=bool)
    if not ok.any():
        return q_err, t_err
    take = lambda a: np.stack([np.asarray(a[b], dtype=np.float64).reshape(-1) for b in np.nonzero(ok)[0]])
    q, t, gq, gt = take(qvecs), take(tvecs), take(gt_qvecs), take(gt_tvecs)
    c = -np.einsum("bji,bj->bi", _rotations(q), t)
    gc = -np.einsum("bji,bj->bi", _rotations(gq), gt)
    t_err[ok] = np.sqrt(np.sum((c - gc) ** 2, axis=1))
    # arccos near 1 magnifies the dot product's last bit by 1 / sin: np.dot per query, the reference's own summation
    d = np.minimum(1.0, np.abs(np.array([np.dot(a, b) for a, b in zip(q, gq)])))
    q_err[ok] = 2 * np.arccos(d) * 180 / np.pi
    return q_err, t_err


RECALL_BARS = ((5.0, 0.05), (2.0, 0.25), (5.0, 0.5), (10.0, 5.0))      # (degrees, metres), loc_by_rec_eval.py:272-279


def recall_counts(q_err, t_err) -> np.ndarray:
    """The four counters of loc_by_rec_eval.py:272-279: queries with q_err <= deg and t_err <= m, both inclusive -> int64 [4]."""
    q, t = np.asarray(q_err, dtype=np.float64).reshape(-1), np.asarray(t_err, dtype=np.float64).reshape(-1)
    return np.array([int(np.sum((q <= dq) & (t <= dt))) for dq, dt in RECALL_BARS], dtype=np.int64)
