"""Candidate-landmark matching on the device: from the recogniser's vote to 2D-3D matches.

Reference: the loop of MultiMap3D.run (localization/multimap3d.py:110-145) around SingleMap3D.localize_with_ref_frame
(localization/singlemap3d.py:127-162) with check_semantic_consistency (singlemap3d.py:513-532) and RefFrame.get_keypoints /
get_keypoints_by_sid (localization/refframe.py:34-75): per query, for each of the seg_k best-voted landmarks, the query keypoints
voted to it are matched against that landmark's reference frame and matches0 becomes (keypoint, xyz) lists for a pose solver.
The reference does this in a host loop with a host <-> device round trip per candidate; here the reference frames are resident
(ReferenceStore), the pairs of ALL queries are planned and gathered by HIP kernels (csrc/candidates.hip), matched in ONE grouped
produce_matches call, and the correspondences are compacted on the device.  The pose solver is pram_amd.localization.pose."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from pram_amd import ops
from pram_amd.nets.utils import keypoint_norm_constants

_FRAME_KEYS = ("keypoints", "descriptors", "xyzs", "point3D_ids", "keypoint_segs", "width", "height")


class StoreBase:
    """What ReferenceStore and MultiMapStore share: the host views over the concatenated arrays, the per-point values (checked on
    first use) and the resident device tables.  A subclass fills the arrays named in _TABLES / _PADDED (and in the hooks below)
    in its constructor, ends it with _ready(device), and says in _point_values where pt_xyz / pt_desc / pt_sid come from."""

    _TABLES = ("descriptors", "keypoints", "scores", "xyzs", "point3D_ids", "keypoint_segs", "frame_norm")
    _PADDED = ("sel_rows", "hist_label", "hist_cnt", "lm_frame", "lm_sel_off", "lm_sel_len", "frame_off", "hist_off",
               "pt_ids", "pt_off", "pt_frames", "is_vrf", "covis_off", "covis_frames", "covis_count")
    _POINT_TABLES = ("pt_xyz", "pt_desc", "pt_sid")
    _EXTRA_PADDED: tuple = ()      # the hooks: further arrays uploaded like _PADDED, further attributes handed over as they are
    _EXTRA_COUNTS: tuple = ()
    _pt_values: Optional[dict] = None

    def _ready(self, device) -> None:
        self._dev: Dict[str, dict] = {}
        self._dev_points: Dict[str, dict] = {}
        if device is not None:
            self.tables(device)

    pt_xyz = property(lambda self: self._point_values()["pt_xyz"])
    pt_desc = property(lambda self: self._point_values()["pt_desc"])
    pt_sid = property(lambda self: self._point_values()["pt_sid"])

    def covisible(self, frame: int) -> np.ndarray:
        """covisible_graph[frame]: the store indices of the frames covisible with store frame `frame`, best first (empty for a
        frame that is no landmark's reference frame)."""
        return self.covis_frames[self.covis_off[frame]:self.covis_off[frame + 1]].astype(np.int64)

    # ---- host views (what the two RefFrame accessors select; used by the tests and by anyone who wants to look)
    @property
    def n_frames(self) -> int:
        return len(self.frame_ids)

    @property
    def n_rows(self) -> int:
        return int(self.frame_off[-1])

    @property
    def max_frame_rows(self) -> int:
        return int(np.diff(self.frame_off).max()) if self.n_frames else 0

    def rows(self, frame: int) -> np.ndarray:
        """RefFrame.get_keypoints: the frame's rows (indices into the concatenated arrays), original order."""
        return np.arange(self.frame_off[frame], self.frame_off[frame + 1], dtype=np.int64)

    def rows_by_sid(self, frame: int, sid: int) -> np.ndarray:
        """RefFrame.get_keypoints_by_sid(sid): the frame's rows with keypoint_segs == sid (an IN-MAP landmark id), original order."""
        off, n = self._slices[frame].get(int(sid), (0, 0))
        return self.sel_rows[off:off + n].astype(np.int64)

    @staticmethod
    def _upload(a: np.ndarray, device, pad: bool) -> torch.Tensor:
        """The pad-and-upload rule: never an empty allocation behind a pointer.  pad: one zero row more; otherwise one zero row
        only where the array has none."""
        zero = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
        a = np.concatenate([a, zero]) if pad else (a if a.size else zero)
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    def tables(self, device) -> dict:
        """The device-side tables (uploaded on first use, then resident)."""
        device = torch.device(device)
        if device.type != "cuda":
            from pram_amd._lib import PramHipError
            raise PramHipError("ReferenceStore.tables: expected a CUDA device (pram_amd has no CPU path)")
        key = str(device)
        if key not in self._dev:
            t = {name: self._upload(getattr(self, name), device, False) for name in self._TABLES}
            t.update({name: self._upload(getattr(self, name), device, True) for name in self._PADDED + self._EXTRA_PADDED})
            t.update(n_rows=self.n_rows, n_frames=self.n_frames, n_landmarks=len(self.lm_frame), start_sid=self.start_sid,
                     n_points=len(self.pt_ids), n_pt_entries=len(self.pt_frames), n_covis=len(self.covis_frames),
                     covisibility_frame=self.covisibility_frame, **{name: getattr(self, name) for name in self._EXTRA_COUNTS})
            self._dev[key] = t
        return self._dev[key]

    def point_tables(self, device) -> dict:
        """tables() plus the per-point values pt_xyz, pt_desc, pt_sid (uploaded on first use, then resident, padded like the
        others): what the refinement by projection reads."""
        t = self.tables(device)
        key = str(torch.device(device))
        if key not in self._dev_points:
            self._dev_points[key] = {**t, **{name: self._upload(getattr(self, name), t["pt_ids"].device, True) for name in self._POINT_TABLES}}
        return self._dev_points[key]


class ReferenceStore(StoreBase):
    """The reference frames of ONE map, built once from plain numpy and uploaded once.

    frames: a sequence of dicts with ``keypoints`` [n, 3] (x, y, score), ``descriptors`` [n, 128], ``xyzs`` [n, 3] float64,
    ``point3D_ids`` [n] int64, ``keypoint_segs`` [n] (in-map landmark id of each keypoint's 3D point), ``width``, ``height`` and
    optionally ``id`` (default: the position in the sequence).  seg_ref_frame_ids: in-map landmark id -> frame ids (a dict or a
    sequence; like the reference, entry [0] is the landmark's reference frame).  start_sid: the map's first global landmark id
    (multimap3d.py:119-123).

    Layout: all rows concatenated in frame order and, inside a frame, in their original order; frame f owns rows
    frame_off[f] .. frame_off[f + 1] (RefFrame.get_keypoints = that range).  ``sel_rows`` holds, per frame, the frame's rows
    stably sorted by keypoint_segs, so get_keypoints_by_sid(sid) = one slice of it (rows with keypoint_segs == sid in their
    original order); the slice of every landmark in its own reference frame is tabulated for the device (lm_sel_off / lm_sel_len).
    Per frame the label histogram that check_semantic_consistency needs (hist_label / hist_cnt).

    For the refinement (localization/refine.py; singlemap3d.py:228-258, 500-511): point3D_frame_ids, a dict from point id to the
    frame ids observing it (COLMAP's image_ids; duplicates are kept and counted, ids of frames outside the store are dropped);
    None derives it from the rows (the frames holding a row with that id, one entry per such row, ascending frame index).  It
    becomes the sorted point table pt_ids with the CSR lists pt_off / pt_frames (store frame indices).  is_vrf marks the frames
    named ANYWHERE in seg_ref_frame_ids; for each of them the covisibility graph (covis_off / covis_frames / covis_count, CSR
    over all frames, empty for the others) lists the covisibility_frame frames sharing most points with it: per row of the frame
    with a known point id (not -1), every frame of that point's list counts once, the frame itself included.  Where the reference
    leaves ties to argsort / argpartition the order here is (count descending, store frame index ascending), at the cut too.

    For the refinement by projection (singlemap3d.py:387-399 reads point3Ds[pid].xyz / .descriptor / .seg_id): point3D_xyzs,
    point3D_descriptors, point3D_sids, dicts from point id to value, become pt_xyz [n_points, 3] float64, pt_desc [n_points, 128]
    float32 and pt_sid [n_points] int32, aligned with pt_ids.  A point a dict does not name (None: every point) takes the value of
    the first row, in store order, that carries its id (the row's xyz, descriptor and keypoint_segs); a point that neither covers
    is a ValueError — raised by the constructor when one of the three arguments is given, and otherwise where the values are
    first asked for (a point table that only votes may name points without rows).  point_tables() uploads them; tables() keeps
    the keys it had."""

    def __init__(self, frames: Sequence[dict], seg_ref_frame_ids, start_sid: int = 0, device=None, *, point3D_frame_ids=None,
                 covisibility_frame: int = 20, point3D_xyzs=None, point3D_descriptors=None, point3D_sids=None):
        frames = list(frames)
        for i, f in enumerate(frames):
            missing = [k for k in _FRAME_KEYS if k not in f]
            if missing:
                raise ValueError(f"reference frame {i}: missing {missing}")
        self.frame_ids = [f.get("id", i) for i, f in enumerate(frames)]
        index_of = {fid: i for i, fid in enumerate(self.frame_ids)}
        if len(index_of) != len(frames):
            raise ValueError("reference frame ids are not unique")
        self.start_sid = int(start_sid)
        lens = [int(np.asarray(f["keypoints"]).shape[0]) for f in frames]
        self.frame_off = np.zeros(len(frames) + 1, dtype=np.int32)
        self.frame_off[1:] = np.cumsum(lens)
        cat = lambda key, dt, shape: (np.concatenate([np.asarray(f[key], dtype=dt).reshape(shape) for f in frames]) if frames
                                      else np.zeros(shape, dtype=dt).reshape((0,) + tuple(shape[1:])))
        kp = cat("keypoints", np.float32, (-1, 3))
        self.keypoints = np.ascontiguousarray(kp[:, :2])
        self.scores = np.ascontiguousarray(kp[:, 2])
        self.descriptors = cat("descriptors", np.float32, (-1, 128))
        self.xyzs = cat("xyzs", np.float64, (-1, 3))
        self.point3D_ids = cat("point3D_ids", np.int64, (-1,))
        self.keypoint_segs = cat("keypoint_segs", np.int32, (-1,))
        n_rows = int(self.frame_off[-1])
        for name in ("descriptors", "xyzs", "point3D_ids", "keypoint_segs"):
            if getattr(self, name).shape[0] != n_rows:
                raise ValueError(f"{name}: row count differs from keypoints")
        self.frame_size = np.array([[int(f["width"]), int(f["height"])] for f in frames], dtype=np.int32).reshape(-1, 2)
        # the matcher call sites hand over (1, 3, width, height) and normalize_keypoints unpacks height, width (singlemap3d.py:152)
        self.frame_norm = np.array([keypoint_norm_constants((1, 3, int(w), int(h))) for w, h in self.frame_size], dtype=np.float32).reshape(-1, 3)
        sel, hoff, hlab, hcnt, self._slices = [], [0], [], [], []
        for f in range(len(frames)):
            a, b = int(self.frame_off[f]), int(self.frame_off[f + 1])
            segs = self.keypoint_segs[a:b]
            order = np.argsort(segs, kind="stable")
            labels, first, cnt = np.unique(segs[order], return_index=True, return_counts=True)
            self._slices.append({int(l): (a + int(s), int(c)) for l, s, c in zip(labels, first, cnt)})
            sel.append(order.astype(np.int32) + a)
            hlab.append(labels.astype(np.int32))
            hcnt.append(cnt.astype(np.int32))
            hoff.append(hoff[-1] + len(labels))
        i32 = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
        self.sel_rows, self.hist_label, self.hist_cnt = i32(sel), i32(hlab), i32(hcnt)
        self.hist_off = np.array(hoff, dtype=np.int32)
        items = seg_ref_frame_ids.items() if isinstance(seg_ref_frame_ids, dict) else enumerate(seg_ref_frame_ids)
        items = [(int(k), v) for k, v in items]
        n_lm = max([k for k, _ in items], default=-1) + 1
        self.lm_frame = np.full(n_lm, -1, dtype=np.int32)
        self.lm_sel_off = np.zeros(n_lm, dtype=np.int32)
        self.lm_sel_len = np.zeros(n_lm, dtype=np.int32)
        for k, v in items:
            if k < 0:
                raise ValueError(f"landmark id {k} < 0")
            v = np.atleast_1d(np.asarray(v))
            if v.size == 0:
                continue
            fid = v[0].item()
            if fid not in index_of:
                raise ValueError(f"landmark {k}: reference frame {fid!r} is not in the store")
            f = index_of[fid]
            self.lm_frame[k] = f
            self.lm_sel_off[k], self.lm_sel_len[k] = self._slices[f].get(k, (0, 0))
        self.covisibility_frame = int(covisibility_frame)
        if self.covisibility_frame < 1:
            raise ValueError("covisibility_frame < 1")
        self.is_vrf = np.zeros(len(frames), dtype=np.int32)
        for _, v in items:
            for fid in np.atleast_1d(np.asarray(v)).tolist():
                if fid in index_of:      # singlemap3d.py:91-92: vrf frames the map does not hold are passed over
                    self.is_vrf[index_of[fid]] = 1
        self._build_point_table(point3D_frame_ids, index_of)
        self._build_covisibility()
        # a store whose point table names points without rows (a vote-only table) stays valid as long as nobody asks for the
        # per-point values: without the three arguments they are derived, and checked, on first use
        self._pt_given = (point3D_xyzs, point3D_descriptors, point3D_sids)
        if any(g is not None for g in self._pt_given):
            self._point_values()
        self._ready(device)

    def _build_point_table(self, point3D_frame_ids, index_of) -> None:
        F = len(self.frame_ids)
        row_frame = np.repeat(np.arange(F, dtype=np.int32), np.diff(self.frame_off))
        if point3D_frame_ids is None:
            rows = np.nonzero(self.point3D_ids != -1)[0]
            self.pt_ids, inv = np.unique(self.point3D_ids[rows], return_inverse=True)
            order = np.argsort(inv.reshape(-1), kind="stable")      # rows are in ascending frame order already
            self.pt_frames = row_frame[rows][order].astype(np.int32)
            lens = np.bincount(inv.reshape(-1), minlength=len(self.pt_ids))
        else:
            keys = np.fromiter((int(k) for k in point3D_frame_ids.keys()), dtype=np.int64, count=len(point3D_frame_ids))
            if len(np.unique(keys)) != len(keys):
                raise ValueError("point3D_frame_ids: point ids are not unique")
            vals = [np.atleast_1d(np.asarray(v)).reshape(-1) for v in point3D_frame_ids.values()]
            lens = np.array([v.shape[0] for v in vals], dtype=np.int64)
            flat = np.concatenate(vals) if vals and lens.sum() else np.zeros(0, dtype=np.int64)
            fids = np.asarray(self.frame_ids)
            if fids.dtype.kind in "iu" and flat.dtype.kind in "iu" and F:
                srt = np.argsort(fids, kind="stable")
                pos = np.clip(np.searchsorted(fids[srt], flat), 0, F - 1)
                fidx = np.where(fids[srt][pos] == flat, srt[pos], -1)
            else:
                fidx = np.array([index_of.get(x, -1) for x in flat.tolist()], dtype=np.int64).reshape(-1)
            owner = np.repeat(np.argsort(np.argsort(keys, kind="stable"), kind="stable"), lens)      # rank of the entry's point
            keep = (fidx >= 0) & np.repeat(keys != -1, lens)
            owner, fidx = owner[keep], fidx[keep]
            order = np.argsort(owner, kind="stable")
            known = np.sort(keys)
            lens = np.bincount(owner, minlength=len(keys))[known != -1]
            self.pt_ids = known[known != -1]
            self.pt_frames = fidx[order].astype(np.int32)
        self.pt_ids = np.ascontiguousarray(self.pt_ids, dtype=np.int64)
        self.pt_off = np.zeros(len(self.pt_ids) + 1, dtype=np.int32)
        self.pt_off[1:] = np.cumsum(lens)

    def _point_values(self) -> dict:
        if self._pt_values is not None:
            return self._pt_values
        xyzs, descriptors, sids = self._pt_given
        out = {}
        n = len(self.pt_ids)
        rows = np.nonzero(self.point3D_ids != -1)[0]
        pi = np.searchsorted(self.pt_ids, self.point3D_ids[rows])
        ok = pi < n
        ok[ok] = self.pt_ids[pi[ok]] == self.point3D_ids[rows][ok]
        has, at = np.unique(pi[ok], return_index=True)      # the first row, in store order, of every point that has one
        first = rows[ok][at]
        index_of = {int(p): i for i, p in enumerate(self.pt_ids.tolist())}
        for name, given, src, dt, tail in (("pt_xyz", xyzs, self.xyzs, np.float64, (3,)), ("pt_desc", descriptors, self.descriptors, np.float32, (128,)),
                                           ("pt_sid", sids, self.keypoint_segs, np.int32, ())):
            val = np.zeros((n,) + tail, dtype=dt)
            covered = np.zeros(n, dtype=bool)
            val[has], covered[has] = src[first], True
            for pid, v in (given or {}).items():
                i = index_of.get(int(pid))
                if i is not None:      # ids outside the point table are passed over
                    val[i], covered[i] = np.asarray(v, dtype=dt).reshape(tail), True
            if not covered.all():
                raise ValueError(f"{name}: {int((~covered).sum())} points of the point table have neither a value nor a row, "
                                 f"e.g. point id {int(self.pt_ids[np.argmin(covered)])}")
            out[name] = val
        self._pt_values = out
        return out

    def _build_covisibility(self) -> None:
        """build_covisibility_graph (singlemap3d.py:228-258) for all vrf frames at once: every (row of a vrf frame, entry of its
        point's frame list) is one count for the pair (frame, listed frame)."""
        F = len(self.frame_ids)
        row_frame = np.repeat(np.arange(F, dtype=np.int64), np.diff(self.frame_off))
        rows = np.nonzero(self.is_vrf[row_frame].astype(bool) & (self.point3D_ids != -1))[0] if F else np.zeros(0, dtype=np.int64)
        pi = np.searchsorted(self.pt_ids, self.point3D_ids[rows])
        ok = pi < len(self.pt_ids)
        ok[ok] = self.pt_ids[pi[ok]] == self.point3D_ids[rows][ok]
        rows, pi = rows[ok], pi[ok]
        lens = (self.pt_off[pi + 1] - self.pt_off[pi]).astype(np.int64)
        start = np.cumsum(lens) - lens
        ent = np.repeat(self.pt_off[pi].astype(np.int64) - start, lens) + np.arange(int(lens.sum()), dtype=np.int64)
        key, cnt = np.unique(np.repeat(row_frame[rows], lens) * max(F, 1) + self.pt_frames[ent], return_counts=True)
        f, g = key // max(F, 1), key % max(F, 1)
        order = np.lexsort((g, -cnt, f))      # per frame: count descending, frame index ascending
        f, g, cnt = f[order], g[order], cnt[order]
        first = np.zeros(F + 1, dtype=np.int64)
        first[1:] = np.cumsum(np.bincount(f, minlength=F))
        keep = np.arange(len(f)) - first[f] < self.covisibility_frame
        f, g, cnt = f[keep], g[keep], cnt[keep]
        self.covis_off = np.zeros(F + 1, dtype=np.int32)
        self.covis_off[1:] = np.cumsum(np.bincount(f, minlength=F))
        self.covis_frames, self.covis_count = g.astype(np.int32), cnt.astype(np.int32)


def _query_norm(features: dict):
    if "image_size" in features:
        w, h = features["image_size"]
    elif "image" in features:
        h, w = features["image"].shape[-2:]
    else:
        raise ValueError("features: needs 'image_size' = (width, height) of the query camera, or the 'image' batch")
    return keypoint_norm_constants((1, 3, int(w), int(h)))      # the reference's (1, 3, width, height), singlemap3d.py:147


@torch.no_grad()
def vote_candidates(features: dict, recognition, seg_k: int) -> dict:
    """Sort + landmark vote for the whole batch (ops.row_sort_desc, ops.seg_vote: the kernels process_segmentations uses).
    recognition: the [B, N, C] segmentations of the batch (a tensor, or a dict with 'segmentations' / 'prediction' and optionally
    'seg_ids' = Frame.seg_ids, e.g. QueryPipeline's 'landmark'), or an already computed vote (a dict with win_sid, win_count, n_win,
    tokens, seg_ids, n_class).  -> dict(win_sid, win_count [B, seg_k], n_win [B], tokens [B, seg_k, N], seg_ids [B, N], n_class)."""
    counts = features["counts"]
    if isinstance(recognition, dict) and "win_sid" in recognition:
        return recognition
    seg_ids = None
    if isinstance(recognition, dict):
        seg_ids = recognition.get("seg_ids")
        recognition = recognition["segmentations"] if "segmentations" in recognition else recognition["prediction"]
    ops._chk(recognition, "recognition")
    seg = recognition.contiguous()
    if seg.dim() != 3 or seg.shape[0] != counts.numel():
        raise ValueError("recognition: expected [B, N, C] with B = len(counts)")
    vals, idx = ops.row_sort_desc(seg)
    ops.cand_mask_ranks_(idx, counts)
    sid, _, cnt, nwin, tokens, _ = ops.seg_vote_batched(vals, idx, seg_k)
    if seg_ids is None:
        seg_ids = ops.seg_epilogue(seg, counts, 2.0)[0]      # argmax - 1 (frame.py:96-121)
    return {"win_sid": sid, "win_count": cnt, "n_win": nwin, "tokens": tokens, "seg_ids": seg_ids.contiguous(), "n_class": seg.shape[2]}


@torch.no_grad()
def plan_candidates(features: dict, recognition, store: StoreBase, *, seg_k: int, min_kpts: int, semantic_matching: bool = True,
                    overlap_ratio: float = 0.5) -> dict:
    """Vote + pram_cand_plan.  -> dict(plan int32 [10, B * seg_k] on the device (ops.CAND_PLAN_FIELDS), vote)."""
    counts = features["counts"]
    ops._chk(counts, "counts", torch.int32)
    v = vote_candidates(features, recognition, seg_k)
    plan = ops.cand_plan(v["win_sid"], v["win_count"], v["n_win"], v["seg_ids"], counts.contiguous(), v["n_class"], store.tables(counts.device),
                         min_kpts, overlap_ratio, semantic_matching)
    return {"plan": plan, "vote": v}


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def padded_size(n0: int, n1: int) -> int:
    """The padded size T of a grouped matcher call whose longest sides have n0 and n1 rows: rounded up to 64, at least 64."""
    return max(64, _round_up(max(n0, n1), 64))


def grouped_inputs(data: dict, plan: torch.Tensor) -> dict:
    """pram_cand_gather's filled dict -> the matcher's data dict, in place: the normalised keypoints under the names the matcher
    reads and the lens0 / lens1 columns of the plan table."""
    f = ops.CAND_PLAN_FIELDS
    data["keypoints0"], data["keypoints1"] = data["norm_keypoints0"], data["norm_keypoints1"]
    data["lens0"], data["lens1"] = plan[f.index("lens0")], plan[f.index("lens1")]
    return data


@torch.no_grad()
def match_grouped(data: dict, plan: torch.Tensor, matcher) -> dict:
    """ONE grouped produce_matches call for all pairs of a plan table (the candidates', the refinement's, the tracker's) on
    pram_cand_gather's filled dict.  matcher: the nn.Module or its localization.matchers wrapper.  -> the matcher's outputs."""
    net = getattr(matcher, "net", matcher)
    return net.produce_matches(grouped_inputs(data, plan))      # its own precision / range-guard scopes (nets/_blocks.with_model_precision)


@torch.no_grad()
def gather_candidates(features: dict, planned: dict, store: StoreBase) -> dict:
    """The ONE host synchronisation of the call: the plan table (40 bytes per pair) is read back to fix the padded size of the
    grouped call — T = max(lens0, lens1) over the pairs, rounded up to 64 — then pram_cand_gather fills the matcher's inputs.
    -> the matcher's data dict plus 'plan_host' (numpy [10, P]) and 't0' (largest query side)."""
    plan = planned["plan"]
    host = plan.cpu().numpy()
    f = ops.CAND_PLAN_FIELDS
    t0, t1 = int(host[f.index("lens0")].max(initial=0)), int(host[f.index("lens1")].max(initial=0))
    data = ops.cand_gather(plan, planned["vote"]["tokens"], store.tables(plan.device), features["descriptors"], features["keypoints"], features["scores"],
                           _query_norm(features), padded_size(t0, t1))
    grouped_inputs(data, plan)
    data["plan_host"], data["t0"] = host, t0
    return data


@torch.no_grad()
def _match_pairs(features: dict, recognition, store: StoreBase, matcher, *, seg_k: int, min_kpts: int, semantic_matching: bool,
                 overlap_ratio: float):
    """The stages of match_candidates up to the compacted correspondences (ONE host synchronisation, the plan read-back).
    -> (cor: pram_cand_correspond's padded outputs [P, t0, ...] and count [P], host: the plan table as numpy [10, P],
    m: the matcher's outputs)."""
    planned = plan_candidates(features, recognition, store, seg_k=seg_k, min_kpts=min_kpts, semantic_matching=semantic_matching,
                              overlap_ratio=overlap_ratio)
    return _match_planned(features, planned, store, matcher)


@torch.no_grad()
def _match_planned(features: dict, planned: dict, store: StoreBase, matcher):
    """_match_pairs from a plan table on: gather, ONE grouped matcher call, correspondences.  The refinement hands its own plan
    over (localization/refine.py); planned = dict(plan, vote = dict(tokens))."""
    data = gather_candidates(features, planned, store)
    host, t0 = data.pop("plan_host"), data.pop("t0")
    plan = planned["plan"]
    m = match_grouped(data, plan, matcher)
    # a batch without a single query keypoint (t0 = 0): an empty slice has no storage to hand over, so one column is passed — no
    # pair reads it (every lens0 is 0) and the outputs keep their cap of t0 rows
    cor = ops.cand_correspond(m["matches0"][:, :max(t0, 1)], plan, planned["vote"]["tokens"], store.tables(plan.device),
                              features["keypoints"].contiguous(), t0)
    return cor, host, m


def _candidate_lists(cor: dict, host, m: dict, store: StoreBase, B: int, seg_k: int) -> List[List[dict]]:
    f = ops.CAND_PLAN_FIELDS
    col = lambda name: host[f.index(name)]
    out: List[List[dict]] = []
    for b in range(B):
        cands = []
        for w in range(seg_k):
            p = b * seg_k + w
            l0, fr = int(col("lens0")[p]), int(col("frame")[p])
            c = {k: cor[k][p, :l0] for k in ops.MATCH_RESULT_KEYS}
            c.update(reference_frame_id=store.frame_ids[fr] if fr >= 0 else None, sid=int(col("sid")[p]),
                     semantic_matching=bool(col("semantic")[p]), n_query_kpts=l0, n_ref_kpts=int(col("lens1")[p]), order=w,
                     n_matches=cor["count"][p], matches0=m["matches0"][p, :l0], matching_scores0=m["matching_scores0"][p, :l0])
            cands.append(c)
        out.append(cands)
    return out


@torch.no_grad()
def match_candidates(features: dict, recognition, store: StoreBase, matcher, *, seg_k: int, min_kpts: int,
                     semantic_matching: bool = True, overlap_ratio: float = 0.5) -> List[List[dict]]:
    """features: the batched extractor output (``keypoints`` [B, N, 2], ``scores`` [B, N], ``descriptors`` [B, N, 128], ``counts``
    int32 [B], all on the GPU, plus ``image_size`` = (width, height) of the query camera or the ``image`` batch); recognition: see
    vote_candidates; matcher: GML / AdaGML (the nn.Module or its localization.matchers wrapper).

    -> per query a list of seg_k candidates in vote order; each a dict with the reference's keys — matched_keypoints [m, 2],
    matched_keypoint_ids [m] int64, matched_xyzs [m, 3] float64, matched_point3D_ids [m] int64, matched_sids [m] int32,
    matched_ref_keypoints [m, 2] (device tensors), reference_frame_id — plus sid (global, vote id - 1), semantic_matching,
    n_query_kpts, n_ref_kpts, order, and n_matches (0-d int32 device tensor).  The matched_* tensors are padded to m = n_query_kpts
    rows; the first n_matches are valid, in ascending query position (no second synchronisation: ``trim_candidate`` cuts them).
    Candidates beyond the vote's winners (and landmarks without a reference frame) come back empty with reference_frame_id None."""
    cor, host, m = _match_pairs(features, recognition, store, matcher, seg_k=seg_k, min_kpts=min_kpts, semantic_matching=semantic_matching,
                                overlap_ratio=overlap_ratio)
    return _candidate_lists(cor, host, m, store, features["counts"].numel(), seg_k)


def trim_candidate(c: dict) -> dict:
    """Cut a candidate's matched_* tensors to their n_matches valid rows (reads one int from the device: synchronises)."""
    n = int(c["n_matches"].item())
    return {k: (v[:n] if k.startswith("matched_") else v) for k, v in c.items()}
