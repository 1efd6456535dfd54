"""Writes tests/golden/prefilter_pinned.npz: what the REFERENCE's Frame.add_segmentations (localization/frame.py:96-121) keeps of
a frame, and what Frame.compute_pose_error (frame.py:139-152) and utils.compute_pose_error (localization/utils.py:39-53) report,
on tests/localizer_ref.py::pinned_cases / pinned_poses.

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are); never runs in
the test suite.  pycolmap is a stand-in module, the Frame objects are built with __new__, a frame's keypoints carry their own row
number so the rows the reference keeps can be read off them.  The fixture holds data only: the logits and thresholds, the kept
rows and seg_ids, the pose pairs and their errors.  The cases regenerate from the seed.

    python tests/tools/gen_prefilter_pinned.py
"""
from __future__ import annotations

import contextlib
import io
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import gen_golden as G  # noqa: E402
from tests import localizer_ref as LR  # noqa: E402


def main():
    G.import_reference()
    G._stub_missing_modules()
    from localization.frame import Frame
    from localization import utils as ref_utils
    cases = LR.pinned_cases(LR.PINNED_SEED)
    out = {"seed": LR.PINNED_SEED, "n_cases": len(cases)}
    fired = {True: 0, False: 0}
    for i, c in enumerate(cases):
        n, th, logits = c["n"], c["threshold"], c["logits"]
        if n and th > 0:      # the mask must not hang on the softmax's last bit
            margin = float(np.abs(LR.softmax64(logits)[:, 0] - th).min())
            assert margin >= LR.PINNED_MARGIN, (i, margin)
        f = Frame.__new__(Frame)
        f.keypoints = np.stack([np.arange(n, dtype=np.float64)] * 3, 1).reshape(n, 3)
        f.descriptors = np.arange(n, dtype=np.float64).reshape(n, 1) * np.ones((1, 4))
        f.initialize_localization_variables = lambda: None
        with contextlib.redirect_stdout(io.StringIO()):
            f.add_segmentations(torch.from_numpy(logits.copy()), th)
        kept = f.keypoints[:, 0].astype(np.int64)
        assert np.array_equal(f.descriptors[:, 0].astype(np.int64), kept) and f.segmentations.shape[0] == len(kept)
        assert np.array_equal(f.segmentations, logits[kept])
        out[f"case{i}_logits"], out[f"case{i}_threshold"] = logits, np.float64(th)
        out[f"case{i}_kept"], out[f"case{i}_seg_ids"] = kept.astype(np.int32), np.asarray(f.seg_ids).astype(np.int32).reshape(-1)
        fired[len(kept) < n or (n == 0 and th > 0)] += 1
        print(f"  case {i}: n {n} threshold {th}: kept {len(kept)}")
    assert len(out[f"case{len(cases) - 4}_kept"]) == 2 and len(out[f"case{len(cases) - 3}_kept"]) == 5      # 2 of 5 fires, 1 of 5 does not
    assert len(out[f"case{len(cases) - 2}_kept"]) == 2 and len(out[f"case{len(cases) - 1}_kept"]) == 5
    assert fired[True] > 5 and fired[False] > 5
    # ---- the evaluation helpers
    qs, ts, gqs, gts = LR.pinned_poses(LR.PINNED_SEED)
    B = len(qs)
    has = np.array([q is not None and t is not None for q, t in zip(qs, ts)])
    fill = lambda rows, k: np.stack([np.zeros(k) if r is None else np.asarray(r, dtype=np.float64) for r in rows])
    q_err, t_err = np.zeros(B), np.zeros(B)
    for b in range(B):
        f = Frame.__new__(Frame)
        f.qvec, f.tvec, f.gt_qvec, f.gt_tvec = qs[b], ts[b], gqs[b], gts[b]
        e = f.compute_pose_error()
        q_err[b], t_err[b] = float(e[0]), float(e[1])
        if has[b]:
            d = ref_utils.compute_pose_error(pred_qcw=qs[b], pred_tcw=ts[b], gt_qcw=gqs[b], gt_tcw=gts[b])
            assert float(d[0]) == q_err[b] and float(d[1]) == t_err[b]
    # the counters live inline in the loop of loc_by_rec_eval.py:272-279 and cannot be called: counted here from the reference's errors
    cnt = [int(np.sum((q_err <= dq) & (t_err <= dt))) for dq, dt in ((5, 0.05), (2, 0.25), (5, 0.5), (10, 5))]
    out.update(pose_has=has, pose_qvecs=fill(qs, 4), pose_tvecs=fill(ts, 3), pose_gt_qvecs=fill(gqs, 4), pose_gt_tvecs=fill(gts, 3),
               pose_q_err=q_err, pose_t_err=t_err, recall=np.array(cnt, dtype=np.int64))
    print(f"  poses: q_err {np.round(q_err, 3).tolist()}\n         t_err {np.round(t_err, 3).tolist()}\n         recall {cnt}")
    G.save("prefilter_pinned", **out)


if __name__ == "__main__":
    main()
