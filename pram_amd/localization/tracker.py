"""Tracking the last frame on the device, for a batch of independent streams.

Reference: Tracker.run / track_last_frame / verify_and_update (localization/tracker.py:37-233) inside the loops of
loc_by_rec_online.py:181-197 and loc_by_rec_eval.py:211-221, with Frame.initialize_localization_variables and update_point3ds
(frame.py:84-89, 191-195).  Once a sequence is located the reference matches the new frame against the PREVIOUS QUERY FRAME —
one matcher pair instead of seg_k — which carries the 3D points its own pose was solved on, solves the pose from those 2D-3D
matches, refines it when it has fewer than 256 inliers, and goes back to the candidate loop only when tracking fails.

Here the last frame of each of S streams lives in a slot of a TrackState on the device.  One ``track`` call serves all queries
of a batch whose stream is not lost: pram_track_plan, pram_cand_gather on the state (unchanged: a tracking pair is a plan row),
ONE grouped produce_matches call, pram_track_correspond, the four pose kernels (seg_k = 1) and ONE read-back of 7 doubles and 3
ints per query.  A tracked query with fewer than ``refine_below`` inliers goes through refine_by_matching / refine_by_projection
— unchanged, on a state dict built from the tracker's own results (chosen = (0, 1, 0), plan = pram_track_plan's loc_plan, est =
the tracker's estimates, cor = the pram_track_filter-ed inlier rows, seg_k = 1) — and is verified again.  ``relocalize`` runs
localize_and_refine (or localize_candidates) on the compact sub-batch of the rest; ``run`` is the two in turn.  A located query
is committed to its slot by pram_track_commit.

Recognition: ``run`` asks for it, ``track`` does not.  The initial seg_ids of a frame never reach a tracking output — only rows
with a point are read from the last frame, and update_point3ds overwrote those with matched_sids — so a host may skip the
recogniser for the streams it expects to track (the state then holds -1 on the rows without a point).

Deviations: the pose stage is pram_amd's (4.12's deviations carry over); the sampler's pair index is the
query's position in the call that solves it (for a relocalised query: its position in the sub-batch); tracker.py:120 sets
``lost = success`` and the loop repairs it (loc_by_rec_online.py:196) — here lost = not success; after a failed tracker the
reference leaves tracking_status False on the frame, MultiMap3D.run tests ``is None`` (multimap3d.py:241) and would go on to
refine an unlocated frame — here a failed tracker hands relocalisation a fresh query; a refinement with success False (or none:
an unknown reference frame) changes nothing, as in 4.13; one map per store; track_last_frame_fast (the bounding-box pre-filter)
is not built; no QueryPipeline stage."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import candidates as _cand
from pram_amd.localization import pose as _pose
from pram_amd.localization import refine as _refine

_LISTS, _COMMIT_KEYS = ops.MATCH_RESULT_KEYS, ops.MATCH_POINT_KEYS


class TrackState:
    """The last frame of n_streams streams on the device, row stride n_max: keypoints [S, n_max, 2], scores [S, n_max],
    descriptors [S, n_max, 128] float32; counts [S] int32; xyzs [S, n_max, 3] float64; point3D_ids [S, n_max] int64 (-1 = no
    point); seg_ids [S, n_max] int32; ref_frame [S] int32 (store index of the frame's reference frame); frame_norm [S, 3] float32
    (normalize_keypoints' constants of the frame's camera).  This is Frame.keypoints / descriptors / xyzs / point3D_ids / seg_ids
    after initialize_localization_variables and update_point3ds.  Only pram_track_commit writes it."""

    def __init__(self, n_streams: int, n_max: int, device):
        S, n_max = int(n_streams), int(n_max)
        if S < 1 or n_max < 1:
            raise ValueError("TrackState: needs n_streams >= 1 and n_max >= 1")
        device = torch.device(device)
        if device.type != "cuda":
            from pram_amd._lib import PramHipError
            raise PramHipError("TrackState: expected a CUDA device (pram_amd has no CPU path)")
        self.n_slots, self.n_max, self.device = S, n_max, device
        z = lambda shape, dt: torch.zeros(shape, device=device, dtype=dt)
        self.keypoints, self.scores, self.descriptors = z((S, n_max, 2), torch.float32), z((S, n_max), torch.float32), z((S, n_max, 128), torch.float32)
        self.counts = z((S,), torch.int32)
        self.xyzs = z((S, n_max, 3), torch.float64)
        self.point3D_ids = torch.full((S, n_max), -1, device=device, dtype=torch.int64)
        self.seg_ids = torch.full((S, n_max), -1, device=device, dtype=torch.int32)
        self.ref_frame = torch.full((S,), -1, device=device, dtype=torch.int32)
        self.frame_norm = torch.tensor([0.0, 0.0, 1.0], device=device).repeat(S, 1).contiguous()

    FIELDS = ("keypoints", "scores", "descriptors", "counts", "xyzs", "point3D_ids", "seg_ids", "ref_frame", "frame_norm")

    def arrays(self) -> dict:
        """What the ops.track_* wrappers take."""
        d = {k: getattr(self, k) for k in self.FIELDS}
        d.update(n_slots=self.n_slots, n_max=self.n_max)
        return d

    def nbytes(self) -> int:
        return sum(getattr(self, k).numel() * getattr(self, k).element_size() for k in self.FIELDS)


# Tracker's keyword options by the stage that takes them: estimate_poses (and every call built on it), localize_candidates' own,
# localize_and_refine's own, and the tracker's switches
OPTION_GROUPS = {"pose": ("threshold", "trials", "min_inlier_ratio", "refine_iters", "seed"),
                 "localize": ("seg_k", "min_kpts", "min_inliers", "semantic_matching", "overlap_ratio"),
                 "refine": ("covisibility_frame", "refinement_method", "projection_min_inliers"),
                 "tracker": ("do_refinement", "refine_below")}
TRACKER_KEYS = tuple(k for keys in OPTION_GROUPS.values() for k in keys)


def split_options(kw: dict, who: str = "Tracker") -> Dict[str, dict]:
    """A dict of Tracker's keyword options (any subset) -> one dict per group of OPTION_GROUPS; a key of no group is a TypeError."""
    unknown = sorted(set(kw) - set(TRACKER_KEYS))
    if unknown:
        raise TypeError(f"{who}: unknown arguments {unknown} (expected Tracker's: {', '.join(TRACKER_KEYS)})")
    return {g: {k: kw[k] for k in keys if k in kw} for g, keys in OPTION_GROUPS.items()}


def _sub_cameras(cameras, idx: Sequence[int]):
    form = _pose.camera_form(cameras)
    if form == "resident":
        t = torch.as_tensor(list(idx), dtype=torch.long, device=cameras[0].device)
        return cameras[0][t].contiguous(), cameras[1][t].contiguous(), [cameras[2][i] for i in idx]
    if form == "table":
        return cameras[0][list(idx)], cameras[1][list(idx)]
    return [cameras[i] for i in idx]


def _sub_recognition(recognition, t: torch.Tensor):
    if torch.is_tensor(recognition):
        return recognition[t].contiguous()
    return {k: (v[t].contiguous() if torch.is_tensor(v) and v.dim() >= 1 and k != "n_class" else v) for k, v in recognition.items()}


class Tracker:
    """The reference's Tracker plus the tracker / relocalisation switch of its loops, for n_streams independent streams.

    store, matcher: as localize_candidates takes them.  seg_k, min_kpts, threshold, min_inliers, semantic_matching, overlap_ratio,
    trials, min_inlier_ratio, refine_iters, seed, covisibility_frame, refinement_method, projection_min_inliers: localize_and_refine's.
    do_refinement: relocalisation refines (multimap3d.py:245-271).  refine_below: a tracked query with fewer inliers is refined
    with ``refinement_method`` (tracker.py:85-94; no 64-inlier gate there).

    ``run`` asks for recognition, ``track`` does not: the initial seg_ids of a frame never reach a tracking output, so a host
    may skip the recogniser for the streams it expects to track (module docstring).

    Per query the calls return a dict: source ('track', 'track+refine', 'relocalize', None = lost), success, qvec (w, x, y, z),
    tvec, num_inliers, inliers (bool [m]), the matched_* device tensors [m, ...], reference_frame_id, tracking (the tracking
    stage's own result, or None) and localization (localize_and_refine's dict, or None).

    Host synchronisations: ``track`` one (plus the refinement's own: two for matching, one for projection, when a query is
    refined); ``relocalize`` those of localize_and_refine."""

    def __init__(self, store, matcher, n_streams: int, n_max: int = 2048, *, seg_k: int, min_kpts: int, threshold: float, min_inliers: int,
                 do_refinement: bool = True, refinement_method: str = "matching", refine_below: int = 256, projection_min_inliers: int = 64,
                 covisibility_frame: Optional[int] = None, trials: int = 1000, semantic_matching: bool = True, overlap_ratio: float = 0.5,
                 min_inlier_ratio: float = 0.01, refine_iters: int = _pose.DEFAULT_REFINE_ITERS, seed: int = 0, device="cuda"):
        given = locals()      # the keyword options by name, before anything else is bound
        opts = split_options({k: given[k] for k in TRACKER_KEYS})
        if refinement_method not in ("matching", "projection"):
            raise NotImplementedError(f"refinement_method {refinement_method!r}")
        self.store, self.matcher = store, matcher
        self.n_streams, self.n_max = int(n_streams), int(n_max)
        self.do_refinement, self.refinement_method, self.refine_below = bool(do_refinement), refinement_method, int(refine_below)
        self.min_inliers, self.threshold = int(min_inliers), float(threshold)
        self._pose_kw, self._loc_kw, self._ref_kw = opts["pose"], {**opts["localize"], **opts["pose"]}, opts["refine"]
        self.covisibility_frame = covisibility_frame
        self.state = TrackState(self.n_streams, self.n_max, device)
        self._dummy = torch.zeros(1, device=self.state.device, dtype=torch.int32)
        self._index_of = {fid: i for i, fid in enumerate(store.frame_ids)}
        self.reset()

    def reset(self, streams=None) -> None:
        """Mark the streams (None: all) lost.  Their slots keep their arrays: a lost slot is never read."""
        if streams is None:
            self.lost = np.ones(self.n_streams, dtype=bool)
            self.qvec: List[Optional[np.ndarray]] = [None] * self.n_streams
            self.tvec: List[Optional[np.ndarray]] = [None] * self.n_streams
            self.reference_frame_id: list = [None] * self.n_streams
            return
        for s in self._streams(streams, len(streams)):
            self.lost[s], self.qvec[s], self.tvec[s], self.reference_frame_id[s] = True, None, None, None

    # ---- helpers
    def _streams(self, streams, B: int) -> List[int]:
        s = list(range(B)) if streams is None else [int(x) for x in (streams.tolist() if hasattr(streams, "tolist") else streams)]
        if len(s) != B:
            raise ValueError("streams: expected one slot per query")
        if any(x < 0 or x >= self.n_streams for x in s) or len(set(s)) != len(s):
            raise ValueError(f"streams: slots must be distinct and inside [0, {self.n_streams})")
        return s

    def _features(self, features: dict):
        counts = features["counts"]
        ops._chk(counts, "counts", torch.int32)
        kp, sc, de = features["keypoints"].contiguous(), features["scores"].contiguous(), features["descriptors"].contiguous()
        if kp.shape[1] > self.n_max:
            raise ValueError(f"features: {kp.shape[1]} keypoints per query exceed the state's n_max = {self.n_max}")
        return counts.contiguous(), kp, sc, de

    def _commit(self, features: dict, members: dict, seg_ids) -> None:
        """members: query index -> (slot, lists (dict of per-query tensors [m, ...]), mask (bool / uint8 [m]) or None, reference frame id)."""
        if not members:
            return
        counts, kp, sc, de = self._features(features)
        B, dev = counts.numel(), counts.device
        cap = max([int(v[1]["matched_keypoint_ids"].shape[0]) for v in members.values()] + [1])
        cor = ops._cor_alloc(B, cap, dev, _COMMIT_KEYS)
        mask = torch.zeros(B, cap, device=dev, dtype=torch.uint8)
        cnt, slot, ref = np.zeros(B, np.int32), np.full(B, -1, np.int32), np.full(B, -1, np.int32)
        for b, (s, lists, inl, fid) in members.items():
            m = int(lists["matched_keypoint_ids"].shape[0])
            for k in _COMMIT_KEYS:
                cor[k][b, :m] = lists[k]
            mask[b, :m] = 1 if inl is None else inl.to(torch.uint8)
            cnt[b], slot[b], ref[b] = m, s, self._index_of.get(fid, -1)
        cor["count"] = torch.from_numpy(cnt).to(dev)
        self._commit_lists(features, cor, mask, slot, ref, seg_ids)

    def _commit_lists(self, features: dict, cor: dict, mask, slot: np.ndarray, ref: np.ndarray, seg_ids) -> None:
        counts, kp, sc, de = self._features(features)
        dev = counts.device
        ops.track_commit(self.state.arrays(), kp, sc, de, counts, None if seg_ids is None else seg_ids.contiguous(), torch.from_numpy(slot).to(dev),
                         slot.tolist(), torch.from_numpy(ref).to(dev), _cand._query_norm(features), cor, mask)

    @staticmethod
    def _result(source=None, src: Optional[dict] = None, tracking=None, localization=None) -> dict:
        """A query's result: located by ``source`` on ``src`` (the stage's dict the pose, the inliers, the lists and the
        reference frame are taken from), or, without src, lost."""
        src = src or {}
        r = {"source": source, "success": bool(src), "qvec": src.get("qvec"), "tvec": src.get("tvec"), "num_inliers": src.get("num_inliers", 0),
             "inliers": src.get("inliers"), "reference_frame_id": src.get("reference_frame_id"), "tracking": tracking, "localization": localization}
        r.update({k: src.get(k) for k in _LISTS})
        return r

    def _record(self, s: int, src: Optional[dict] = None) -> None:
        """A stream's outcome: located on src, or (None) lost — its last pose stays, a lost slot is never read."""
        self.lost[s] = src is None
        if src is not None:
            self.qvec[s], self.tvec[s], self.reference_frame_id[s] = src["qvec"], src["tvec"], src["reference_frame_id"]

    # ---- the tracking branch
    @torch.no_grad()
    def track(self, features: dict, cameras, streams=None, *, seg_ids: Optional[torch.Tensor] = None, image_sizes=None) -> List[Optional[dict]]:
        """The tracking branch alone, for the queries whose stream is not lost; needs no recognition.  seg_ids int32 [B, N]: the
        frames' own landmark labels (Frame.seg_ids), kept on the rows that get no point (None: -1 there).  -> per query None (its
        stream is lost: not tried) or the result dict; a query whose tracking failed comes back with source None, success False and
        ``tracking`` filled in, and its stream is marked lost (``run`` hands it to relocalize)."""
        counts, kp, sc, de = self._features(features)
        B, N, dev = counts.numel(), kp.shape[1], counts.device
        slots = self._streams(streams, B)
        slot = np.array([s if not self.lost[s] else -1 for s in slots], dtype=np.int32)
        out: List[Optional[dict]] = [None] * B
        if B == 0 or N == 0 or (slot < 0).all():
            return out
        st = self.state.arrays()
        plan, loc_plan = ops.track_plan(counts, torch.from_numpy(slot).to(dev), st, N)
        data = ops.cand_gather(plan, self._dummy, ops.track_gather_tables(st, self._dummy), de, kp, sc, _cand._query_norm(features),
                               _cand.padded_size(N, self.n_max))      # known on the host: no plan read-back
        m = _cand.match_grouped(data, plan, self.matcher)
        cor = ops.track_correspond(m["matches0"][:, :N], plan, st, kp, N)
        est = _pose.estimate_poses(cor["matched_keypoints"], cor["matched_xyzs"], cor["count"], cameras, seg_k=1, **self._pose_kw)
        # the one read-back: 7 doubles and 3 ints per query
        rb = _pose.ReadBack(est, {"success": est["success"], "num_inliers": est["num_inliers"], "n_matches": cor["count"]})
        tracked = np.zeros(B, dtype=bool)
        for b in range(B):
            if slot[b] < 0:
                continue
            v = rb[b]
            n = v["n_matches"]
            tracked[b] = bool(v["success"]) and v["num_inliers"] >= self.min_inliers
            t = {"success": bool(v["success"]), "tracked": bool(tracked[b]), "qvec": v["qvec"], "tvec": v["tvec"], "num_inliers": v["num_inliers"],
                 "inliers": est["inliers"][b, :n].bool(), "n_matches": n, "reference_frame_id": self.reference_frame_id[slots[b]],
                 "matches0": m["matches0"][b], "matching_scores0": m["matching_scores0"][b], "refinement": None}
            t.update({k: cor[k][b, :n] for k in _LISTS})
            out[b] = self._result(tracking=t)
        # refinement is necessary for tracking last frame (tracker.py:85-94)
        group = tracked & np.array([out[b] is not None and out[b]["tracking"]["num_inliers"] < self.refine_below for b in range(B)])
        refined: List[Optional[dict]] = [None] * B
        if group.any():
            chosen = torch.from_numpy(np.stack([np.where(tracked, 0, -1), np.ones(B), np.zeros(B)], 1).astype(np.int32)).to(dev)
            state = {"chosen": chosen, "plan": loc_plan, "tokens": self._dummy, "cor": ops.track_filter(cor, est["inliers"]), "est": est, "seg_k": 1}
            kw = dict(self._pose_kw, covisibility_frame=self.covisibility_frame, enable=group.astype(np.int32))
            if self.refinement_method == "matching":
                refined = _refine.refine_by_matching(features, state, self.store, self.matcher, cameras, **kw)
            else:
                refined = _refine.refine_by_projection(features, state, self.store, cameras, image_sizes=image_sizes, **kw)
        direct_slot, members = np.full(B, -1, np.int32), {}
        direct_ref = np.full(B, -1, np.int32)
        for b in range(B):
            if not tracked[b]:
                if slot[b] >= 0:
                    self._record(slots[b])
                continue
            t, x, s = out[b]["tracking"], refined[b] if group[b] else None, slots[b]
            if x is not None:
                x["method"] = self.refinement_method
                t["refinement"] = x
            if x is not None and x["success"]:      # a refinement with success False changes nothing
                if x["num_inliers"] < self.min_inliers:      # verified again (tracker.py:94)
                    tracked[b], t["tracked"] = False, False
                    self._record(s)
                    continue
                out[b] = self._result("track+refine", x, t)
                members[b] = (s, {k: x[k] for k in _COMMIT_KEYS}, x["inliers"], x["reference_frame_id"])
            else:
                out[b] = self._result("track", t, t)
                direct_slot[b], direct_ref[b] = s, self._index_of.get(t["reference_frame_id"], -1)
            self._record(s, out[b])
        # the hand-over: the tracker's inlier rows, or the refinement's (update_current_frame, update_point3ds)
        if (direct_slot >= 0).any():
            self._commit_lists(features, cor, est["inliers"], direct_slot, direct_ref, seg_ids)
        self._commit(features, members, seg_ids)
        return out

    # ---- the fallback
    @torch.no_grad()
    def relocalize(self, features: dict, recognition, cameras, streams=None, which=None, *, image_sizes=None) -> List[dict]:
        """The candidate loop (localize_and_refine, or localize_candidates without do_refinement) on the compact sub-batch of
        the queries ``which`` (indices into the batch; None: all), then the hand-over.  -> one result dict per entry of which."""
        counts, kp, sc, de = self._features(features)
        B, dev = counts.numel(), counts.device
        slots = self._streams(streams, B)
        which = list(range(B)) if which is None else [int(b) for b in which]
        if not which:
            return []
        t = torch.as_tensor(which, dtype=torch.long, device=dev)
        sub = {k: v for k, v in features.items() if k not in ("keypoints", "scores", "descriptors", "counts", "image")}
        sub.update(keypoints=kp[t].contiguous(), scores=sc[t].contiguous(), descriptors=de[t].contiguous(), counts=counts[t].contiguous())
        if "image_size" not in sub:
            w, h = features["image"].shape[-1], features["image"].shape[-2]
            sub["image_size"] = (w, h)
        vote = _cand.vote_candidates(sub, _sub_recognition(recognition, t), self._loc_kw["seg_k"])
        cams = _sub_cameras(cameras, which)
        if self.do_refinement:
            sizes = None if image_sizes is None else torch.as_tensor(np.asarray(image_sizes.cpu() if torch.is_tensor(image_sizes) else image_sizes))[which]
            res = _refine.localize_and_refine(sub, vote, self.store, self.matcher, cams, image_sizes=sizes, **self._loc_kw, **self._ref_kw)
        else:
            res = _pose.localize_candidates(sub, vote, self.store, self.matcher, cams, **self._loc_kw)
        seg_ids = torch.full((B, kp.shape[1]), -1, device=dev, dtype=torch.int32)
        seg_ids[t] = vote["seg_ids"]
        out, members = [], {}
        for b, r in zip(which, res):
            s = slots[b]
            if not r["success"]:
                self._record(s)
                out.append(self._result(localization=r))
                continue
            x = r.get("refinement")
            if x is not None and x["success"]:      # multimap3d.py:259-271: the refinement's inlier rows
                src, inl = x, x["inliers"]
            else:                                    # update_query_frame, multimap3d.py:315-328: ALL matches of the kept candidate
                src, inl = r, None
            out.append(self._result("relocalize", src, None, r))
            members[b] = (s, {k: src[k] for k in _COMMIT_KEYS}, inl, src["reference_frame_id"])
            self._record(s, src)
        self._commit(features, members, seg_ids)
        return out

    @torch.no_grad()
    def run(self, features: dict, recognition, cameras, streams=None, *, image_sizes=None) -> List[dict]:
        """track, then relocalize on what track did not hold (loc_by_rec_online.py:181-197).  B <= n_streams queries, streams[b] =
        the slot of query b (default arange(B))."""
        B = features["counts"].numel()
        seg_ids = frame_seg_ids(features, recognition)
        out = self.track(features, cameras, streams, seg_ids=seg_ids, image_sizes=image_sizes)
        rest = [b for b in range(B) if out[b] is None or not out[b]["success"]]
        for b, r in zip(rest, self.relocalize(features, recognition, cameras, streams, rest, image_sizes=image_sizes)):
            r["tracking"] = None if out[b] is None else out[b]["tracking"]
            out[b] = r
        return out


@torch.no_grad()
def frame_seg_ids(features: dict, recognition) -> torch.Tensor:
    """Frame.seg_ids of the batch (argmax - 1, frame.py:121) from what vote_candidates takes as recognition."""
    if isinstance(recognition, dict):
        if recognition.get("seg_ids") is not None:
            return recognition["seg_ids"].contiguous()
        recognition = recognition["segmentations"] if "segmentations" in recognition else recognition["prediction"]
    ops._chk(recognition, "recognition")
    return ops.seg_epilogue(recognition.contiguous(), features["counts"], 2.0)[0].contiguous()
