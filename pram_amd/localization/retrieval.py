"""Localisation against retrieved database frames, on the device: the reference's offline localizer.

Reference: localization/pose_estimator.py as localization/localizer.py drives it — get_covisibility_frames (:18-42),
feature_matching (:45-86), find_2D_3D_matches (:89-134), pose_estimator_hloc (:138-270), pose_refinement (:273-376) and
pose_estimator_iterative (:380-612).  A query comes with a list of retrieved database frames; every keypoint of the query is
matched against the rows of each frame that carry a 3D point, the matches whose point has too few observations are dropped, and
either ONE pose is solved on all frames' matches stacked ('hloc') or one pose per frame, of which the first with enough inliers
is kept ('iterative'), optionally refined over the frames covisible with the kept one.  The reference does this in a host loop with
a matcher call and a host round trip per (query, frame) pair; here the frames of the SfM model are resident (DatabaseStore), the
pairs of ALL queries are planned by pram_retr_plan, gathered by pram_cand_gather, matched in ONE grouped produce_matches call,
compacted by pram_cand_correspond and pram_retr_filter, stacked by pram_refine_merge, solved by the pose kernels and chosen by
pram_retr_select; covisibility is pram_covis_topk, for any frame of the store.

Host synchronisations of localize_by_retrieval: one plan read-back per grouped matcher call (40 bytes per pair, as
candidates.gather_candidates does it: one call without do_covisibility_opt, two with it) and ONE read-back of the results.

Deviations:
  1. the pose stage is pram_amd's, with a fixed ``trials`` budget (DESIGN.md 4.12's deviations carry over);
  2. 'iterative' matches and solves ALL retrieved frames of a query and then selects, where the reference stops at the first
     accepted frame (:556); pairs are independent, so the result is the same (profiles/retrieval_timing.md has the cost);
  3. where the reference leaves the order of equal covisibility counts to argsort / argpartition (:34-38) the order is (count
     descending, store frame index ascending), at the cut too;
  4. three places where the reference's code is broken have a defined behaviour here: :558-599 without do_covisibility_opt read
     ``ret`` and ``loc_keypoints_query`` left over from the LAST loop iteration — here the best slot's pose and inliers are used
     (with the option: the refinement's, or the best slot's when the refinement fails); :601 ``db_ids[0][0]`` is a TypeError —
     here the result is the first retrieved frame's stored pose with num_inliers -1 (qvec None when the store has no poses); an
     empty retrieval list is an IndexError at :169 / :420 — here success False, qvec None, num_inliers 0; and :515 / :567 call
     pose_refinement without its query_data (a TypeError: the reference cannot run do_covisibility_opt) — here the refinement
     runs on the query's own features, as pose_refinement itself is written;
  5. the + 0.5 of :133 is applied where the pose stage applies it already (pram_pose_prepare): the lists carry the keypoints as
     the extractor gave them, keypoints_query included.
'hloc' fixes obs_th to 3 whatever the caller passes, as the reference does (:182); the caller's obs_th holds for 'iterative' and
for both forms' covisibility stage.  localizer.py's command line, file writing and logging are not built."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from pram_amd import ops
from pram_amd.localization import candidates as _cand
from pram_amd.localization import pose as _pose
from pram_amd.localization.candidates import ReferenceStore

_MATCHED = ops.MATCH_RESULT_KEYS + (ops.MATCH_SRC,)
HLOC_OBS_TH = 3      # pose_estimator.py:182


class DatabaseStore(ReferenceStore):
    """The frames of an SfM model (the reference's db_images, feature file and points3D), resident like a ReferenceStore.

    frames: as ReferenceStore takes them; ``keypoint_segs`` may be left out (zeros: an unlabelled model) and ``xyzs`` too when
    point3D_xyzs names every point.  seg_ref_frame_ids defaults to {} (no landmarks, no reference frames: the store's own
    covisibility graph is then empty, covisible_frames below serves any frame).  point3D_frame_ids: point id -> image ids
    (points3D[id].image_ids; None derives it from the rows).  poses: optional, frame id -> (qvec (w, x, y, z), tvec), or a pair of
    arrays (qvecs [F, 4], tvecs [F, 3]) in frame order; used only where a failed query takes the first retrieved frame's pose.
    from_triangulation builds one straight from triangulation.triangulate_map's (or map_tables') result.

    Added tables: valid_rows / valid_off, per frame the rows (indices into the concatenated arrays, original order) whose point id
    is not -1 and is in the point table — what feature_matching selects with ``db_3D_ids != -1`` (pose_estimator.py:63); n_valid.
    A point's observation count, len(points3D[id].image_ids), is pt_off[i + 1] - pt_off[i] of the point table (observations())."""

    _EXTRA_PADDED = ("valid_rows", "valid_off")
    _EXTRA_COUNTS = ("n_valid",)

    def __init__(self, frames: Sequence[dict], seg_ref_frame_ids=None, start_sid: int = 0, device=None, *, point3D_frame_ids=None,
                 covisibility_frame: int = 20, point3D_xyzs=None, point3D_descriptors=None, point3D_sids=None, poses=None):
        full = []
        for f in frames:
            f = dict(f)
            n = int(np.asarray(f["keypoints"]).shape[0]) if "keypoints" in f else 0
            f.setdefault("keypoint_segs", np.zeros(n, dtype=np.int32))
            if "xyzs" not in f and point3D_xyzs is not None and "point3D_ids" in f:
                zero = np.zeros(3, dtype=np.float64)
                f["xyzs"] = np.array([point3D_xyzs.get(int(p), zero) for p in np.asarray(f["point3D_ids"]).tolist()], dtype=np.float64).reshape(-1, 3)
            full.append(f)
        super().__init__(full, {} if seg_ref_frame_ids is None else seg_ref_frame_ids, start_sid, None, point3D_frame_ids=point3D_frame_ids,
                         covisibility_frame=covisibility_frame, point3D_xyzs=point3D_xyzs, point3D_descriptors=point3D_descriptors,
                         point3D_sids=point3D_sids)
        pi = np.searchsorted(self.pt_ids, self.point3D_ids)
        ok = (self.point3D_ids != -1) & (pi < len(self.pt_ids))
        ok[ok] = self.pt_ids[pi[ok]] == self.point3D_ids[ok]
        self.valid_rows = np.nonzero(ok)[0].astype(np.int32)      # ascending: frame order and, inside a frame, original order
        self.valid_off = np.searchsorted(self.valid_rows, self.frame_off).astype(np.int32)
        self.n_valid = len(self.valid_rows)
        self.index_of = {fid: i for i, fid in enumerate(self.frame_ids)}
        self.poses = self._pose_table(poses)
        self._ready(device)

    def _pose_table(self, poses):
        if poses is None:
            return None
        F = self.n_frames
        if isinstance(poses, dict):
            missing = [fid for fid in self.frame_ids if fid not in poses]
            if missing:
                raise ValueError(f"poses: no pose for frame {missing[0]!r}")
            q = np.array([np.asarray(poses[fid][0], dtype=np.float64).reshape(4) for fid in self.frame_ids]).reshape(F, 4)
            t = np.array([np.asarray(poses[fid][1], dtype=np.float64).reshape(3) for fid in self.frame_ids]).reshape(F, 3)
        else:
            q, t = (np.asarray(x, dtype=np.float64) for x in poses)
            if q.shape != (F, 4) or t.shape != (F, 3):
                raise ValueError("poses: expected (qvecs [F, 4], tvecs [F, 3]) in frame order")
        return q, t

    @classmethod
    def from_triangulation(cls, frames: Sequence[dict], mapped: dict, device=None, *, poses=None, covisibility_frame: int = 20):
        """frames: the feature frames triangulate_map was given (``keypoints`` [n, 3] (x, y, score), ``descriptors``, ``width``,
        ``height``, optionally ``id``); mapped: triangulate_map's (or map_tables') dict, whose ``frames`` carry point3D_ids and xyzs
        and whose point3D_frame_ids are the tracks' image ids."""
        if len(frames) != len(mapped["frames"]):
            raise ValueError("from_triangulation: the map was built from another number of frames")
        merged = [{**f, "point3D_ids": m["point3D_ids"], "xyzs": m["xyzs"]} for f, m in zip(frames, mapped["frames"])]
        return cls(merged, device=device, point3D_frame_ids=mapped["point3D_frame_ids"], poses=poses, covisibility_frame=covisibility_frame)

    def valid(self, frame: int) -> np.ndarray:
        """The rows of store frame `frame` that carry a point of the point table, original order."""
        return self.valid_rows[self.valid_off[frame]:self.valid_off[frame + 1]].astype(np.int64)

    def observations(self, point3D_ids) -> np.ndarray:
        """len(points3D[id].image_ids) per id (duplicates counted); 0 for an id the point table does not hold."""
        ids = np.asarray(point3D_ids, dtype=np.int64).reshape(-1)
        pi = np.clip(np.searchsorted(self.pt_ids, ids), 0, max(len(self.pt_ids) - 1, 0))
        n = np.diff(self.pt_off)
        return np.where(self.pt_ids[pi] == ids, n[pi], 0).astype(np.int64) if len(self.pt_ids) else np.zeros(len(ids), dtype=np.int64)

    def indices(self, frame_ids, what: str = "frame") -> list:
        """frame ids -> store frame indices; an id the store does not hold is a ValueError."""
        out = []
        for fid in frame_ids:
            fid = fid.item() if isinstance(fid, np.generic) else fid
            if fid not in self.index_of:
                raise ValueError(f"{what} {fid!r} is not in the store")
            out.append(self.index_of[fid])
        return out


class _ValidRowsView:
    """The store as the candidate stage's gather and correspond read it, with valid_rows where they look for sel_rows."""

    def __init__(self, store: DatabaseStore):
        self.store = store

    def tables(self, device) -> dict:
        t = self.store.tables(device)
        return {**t, "sel_rows": t["valid_rows"]}


@torch.no_grad()
def covisible_frames(store: DatabaseStore, frame_ids, k: int, include_self: bool = False, device="cuda"):
    """get_covisibility_frames for a list of frame ids at once -> (frames int32 [n, k] store frame INDICES, -1 padded, counts int32
    [n, k], n_found int32 [n]), device tensors; nothing is read back.  Order: count descending, then store frame index ascending.
    The histogram workspace stays under ops.COVIS_WORKSPACE_BYTES (64 MiB): longer lists go through the kernel in chunks."""
    if int(k) < 1:
        raise ValueError("k < 1")
    t = store.tables(device)
    idx = torch.tensor(store.indices(frame_ids), dtype=torch.int32, device=t["valid_rows"].device)
    return ops.covis_topk(idx, t, int(k), include_self)


@torch.no_grad()
def covisibility_pairs(store: DatabaseStore, k: int, device="cuda") -> list:
    """The content of a pairs-db-covis<k>.txt: for every frame of the store, in store order, (frame id, covisible frame id) for its
    k most covisible frames (itself excluded), best first — ready for triangulate_map(pairs=...), unique_pairs and match_pairs
    once the ids are positions.  One read-back."""
    frames, _, n_found = covisible_frames(store, store.frame_ids, k, False, device)
    host = torch.cat([frames, n_found[:, None]], 1).cpu().numpy()
    return [(store.frame_ids[f], store.frame_ids[int(g)]) for f in range(store.n_frames) for g in host[f, :host[f, -1]]]


def _match_plan(features: dict, plan: torch.Tensor, store: DatabaseStore, matcher, obs_th: int):
    """gather, ONE grouped matcher call, correspondences, the observation filter -> (filtered lists, plan on the host, matcher
    outputs).  ONE host synchronisation, the plan read-back."""
    dummy = torch.zeros(1, device=plan.device, dtype=torch.int32)      # tok_off is -1 in every row: no token list is read
    cor, host, m = _cand._match_planned(features, {"plan": plan, "vote": {"tokens": dummy}}, _ValidRowsView(store), matcher)
    return ops.retr_filter(cor, store.tables(plan.device), obs_th), host, m


def _stack(lists: dict, n_slots: int) -> dict:
    """Per query the slots' rows in slot order (all_mkpts / all_mp3ds of pose_estimator_hloc, the lists of pose_refinement):
    pram_refine_merge with init_on all zero, which then reads nothing of its second list."""
    B = lists["count"].numel() // n_slots
    dev = lists["count"].device
    zero = torch.zeros(B, device=dev, dtype=torch.int32)
    return ops.refine_merge(lists, lists, torch.full((B, 3), -1, device=dev, dtype=torch.int32), zero, n_slots)


def _inlier_order(inliers: torch.Tensor) -> torch.Tensor:
    """Per row of uint8 [P, t] the positions of the inliers first, in ascending order: cut to num_inliers on the host, it selects
    the inliers without a read-back."""
    return torch.sort(inliers, dim=1, descending=True, stable=True).indices


def _host(tensors: dict) -> dict:
    """ONE device-to-host copy of several tensors (they travel as float64, which holds every int32 exactly)."""
    flat = torch.cat([t.double().reshape(-1) for t in tensors.values()]).cpu().numpy()
    out, at = {}, 0
    for k, t in tensors.items():
        out[k] = flat[at:at + t.numel()].reshape(t.shape)
        at += t.numel()
    return out


@torch.no_grad()
def localize_by_retrieval(features: dict, retrieval, store: DatabaseStore, matcher, cameras, *, method: str = "hloc", threshold: float = 12.0,
                          obs_th: int = 3, inlier_th: int = 50, min_best_inliers: int = 10, do_covisibility_opt: bool = False,
                          covisibility_frame: int = 50, opt_th: float = 12.0, trials: int = 1000, min_inlier_ratio: float = 0.01,
                          refine_iters: int = _pose.DEFAULT_REFINE_ITERS, seed: int = 0) -> List[dict]:
    """features, matcher, cameras: as localize_candidates takes them; retrieval: per query a sequence of frame ids (ragged; an id
    the store does not hold is a ValueError); store: a DatabaseStore.

    method 'hloc' (pose_estimator_hloc): every (query, retrieved frame) pair matched in ONE grouped call, the rows filtered with
    obs_th 3 — fixed, as in the reference (:182), whatever ``obs_th`` says — stacked in slot order, one pose per query at
    ``threshold``.  method 'iterative' (pose_estimator_iterative): the same grouped call, the rows filtered with ``obs_th``, one pose
    per pair (the sampler's pair index is query * n_db + slot), then pram_retr_select: the first slot with >= 8 rows, a solved
    pose and num_inliers >= inlier_th is accepted; with none, the slot with most inliers is taken when it has min_best_inliers.
    do_covisibility_opt ('iterative' only, as in the reference): for the kept queries the covisibility_frame frames covisible with
    the kept frame (itself excluded) are matched in a second grouped call, filtered with ``obs_th``, stacked and solved as one pose
    at ``opt_th`` (the sampler's pair index is the query index); a refinement whose solver fails keeps the first pose with
    num_inliers 0 and empty inlier lists (:351-363).

    Host synchronisations: one plan read-back per grouped matcher call and ONE read-back of the results.

    -> per query a dict: success, status ('hloc': 1 solved, 0 failed; 'iterative': 1 accepted, 2 best taken, 0 failed), qvec (w, x, y,
    z), tvec, num_inliers, order (-1 for 'hloc', slot + 1 for 'iterative'), reference_frame_id (the reference's dbname: the kept
    frame; the first retrieved frame where none was kept; None for an empty list), keypoints_query [num_inliers, 2] and points3D_ids
    [num_inliers] of the inliers, inliers (bool over the matched lists), the matched_* lists the pose was solved on cut to their
    count (device tensors; 'hloc' and the refinement add matched_src, the slot of origin), and slots: per retrieved frame its
    reference_frame_id, n_query_kpts, n_ref_kpts (valid rows), matches0 / matching_scores0 [n_query_kpts], n_matches (after the
    filter, 0-d device tensor) and for 'iterative' success, num_inliers, qvec, tvec of the slot's own pose.  With
    do_covisibility_opt a kept query also has ``refinement``: success, qvec, tvec, num_inliers, inliers, the stacked lists,
    covisible_frame_ids and slots.  A failed query: success False, num_inliers 0 ('iterative' with a non-empty list: -1) and the
    first retrieved frame's stored pose, or qvec None when the store has no poses or the list is empty."""
    if method not in ("hloc", "iterative"):
        raise ValueError(f"method {method!r}: expected 'hloc' or 'iterative'")
    counts = features["counts"]
    ops._chk(counts, "counts", torch.int32)
    dev, B = counts.device, counts.numel()
    if len(retrieval) != B:
        raise ValueError("retrieval: expected one list of frame ids per query")
    if B == 0:
        return []
    lists = [store.indices(r, "retrieved frame") for r in retrieval]
    n_db = max(1, max(len(l) for l in lists))
    table = np.full((B, n_db), -1, dtype=np.int32)
    for b, l in enumerate(lists):
        table[b, :len(l)] = l
    tables = store.tables(dev)
    counts = counts.contiguous()
    cams = _pose._device_cameras(cameras, dev)
    pose_kw = dict(trials=trials, min_inlier_ratio=min_inlier_ratio, refine_iters=refine_iters, seed=seed)
    table_dev = torch.from_numpy(table).to(dev)
    plan = ops.retr_plan(table_dev, counts, tables)
    hloc = method == "hloc"
    flt, host, m = _match_plan(features, plan, store, matcher, HLOC_OBS_TH if hloc else obs_th)
    f = ops.CAND_PLAN_FIELDS
    col = lambda h, name: h[f.index(name)]

    def slot_list(h, mm, cnt, names, b, n, width):
        out = []
        for j in range(n):
            p = b * width + j
            l0 = int(col(h, "lens0")[p])
            out.append({"reference_frame_id": names[j], "n_query_kpts": l0, "n_ref_kpts": int(col(h, "lens1")[p]), "matches0": mm["matches0"][p, :l0],
                        "matching_scores0": mm["matching_scores0"][p, :l0], "n_matches": cnt[p]})
        return out

    def stored_pose(b):
        if store.poses is None or not lists[b]:
            return None, None
        return store.poses[0][lists[b][0]].copy(), store.poses[1][lists[b][0]].copy()

    def solved(lst, est, order, row, n, n_inl, keys):
        """the entries of a result that come from a solved list: row of lst / est / order, n matched rows, n_inl inliers"""
        sel = order[row, :n_inl]
        r = {"inliers": est["inliers"][row, :n].bool(), "keypoints_query": lst["matched_keypoints"][row][sel],
             "points3D_ids": lst["matched_point3D_ids"][row][sel]}
        r.update({key: lst[key][row, :n] for key in keys})
        return r

    def empty(lst, keys):
        r = {"inliers": None, "keypoints_query": lst["matched_keypoints"][0, :0], "points3D_ids": lst["matched_point3D_ids"][0, :0]}
        r.update({key: lst[key][0, :0] for key in keys})
        return r

    names = [[store.frame_ids[i] for i in l] for l in lists]
    if hloc:
        stack = _stack(flt, n_db)
        est = _pose.estimate_poses(stack["matched_keypoints"], stack["matched_xyzs"], stack["count"], cams, seg_k=1, threshold=threshold, **pose_kw)
        order = _inlier_order(est["inliers"])
        rb = _host({"qvec": est["qvec"], "tvec": est["tvec"], "success": est["success"], "num_inliers": est["num_inliers"], "count": stack["count"]})
        out = []
        for b in range(B):
            ok = bool(rb["success"][b]) and bool(lists[b])
            r = {"success": ok, "status": int(ok), "order": -1, "reference_frame_id": names[b][0] if names[b] else None,
                 "slots": slot_list(host, m, flt["count"], names[b], b, len(lists[b]), n_db)}
            if ok:
                n, n_inl = int(rb["count"][b]), int(rb["num_inliers"][b])
                r.update(qvec=rb["qvec"][b].copy(), tvec=rb["tvec"][b].copy(), num_inliers=n_inl, **solved(stack, est, order, b, n, n_inl, _MATCHED))
            else:      # :188-208, :250-270: the pose of the first retrieved frame as approximation
                q, t = stored_pose(b)
                r.update(qvec=q, tvec=t, num_inliers=0, **empty(stack, _MATCHED))
            out.append(r)
        return out

    est = _pose.estimate_poses(flt["matched_keypoints"], flt["matched_xyzs"], flt["count"], cams, seg_k=n_db, threshold=threshold, **pose_kw)
    chosen = ops.retr_select(est["success"], est["num_inliers"], flt["count"], n_db, inlier_th, min_best_inliers)
    order = _inlier_order(est["inliers"])
    back = {"qvec": est["qvec"], "tvec": est["tvec"], "success": est["success"], "num_inliers": est["num_inliers"], "count": flt["count"], "chosen": chosen}
    if do_covisibility_opt:
        n_cov = int(covisibility_frame)
        if n_cov < 1:
            raise ValueError("covisibility_frame < 1")
        kept = chosen[:, 0].long()
        kept_frame = torch.where(kept >= 0, table_dev.gather(1, kept.clamp(min=0)[:, None])[:, 0],
                                 torch.full((B,), -1, device=dev, dtype=torch.int32)).contiguous()
        cov_frames, _, n_cov_found = ops.covis_topk(kept_frame, tables, n_cov, False)      # a query that kept nothing: frame -1, an empty list
        plan2 = ops.retr_plan(cov_frames.contiguous(), counts, tables)
        flt2, host2, m2 = _match_plan(features, plan2, store, matcher, obs_th)
        stack2 = _stack(flt2, n_cov)
        est2 = _pose.estimate_poses(stack2["matched_keypoints"], stack2["matched_xyzs"], stack2["count"], cams, seg_k=1, threshold=opt_th, **pose_kw)
        order2 = _inlier_order(est2["inliers"])
        back.update(qvec2=est2["qvec"], tvec2=est2["tvec"], success2=est2["success"], num_inliers2=est2["num_inliers"], count2=stack2["count"],
                    cov_frames=cov_frames, n_cov_found=n_cov_found)
    rb = _host(back)      # the one read-back of the results
    out = []
    for b in range(B):
        kept, status, best = (int(x) for x in rb["chosen"][b])
        slots = slot_list(host, m, flt["count"], names[b], b, len(lists[b]), n_db)
        for j, s in enumerate(slots):
            p = b * n_db + j
            s.update(success=bool(rb["success"][p]), num_inliers=int(rb["num_inliers"][p]), qvec=rb["qvec"][p].copy(), tvec=rb["tvec"][p].copy())
        r = {"success": kept >= 0, "status": status, "best_slot": best, "slots": slots}
        if kept < 0:      # :601-612 (no slot was good enough) or an empty list
            q, t = stored_pose(b)
            r.update(qvec=q, tvec=t, num_inliers=-1 if lists[b] else 0, order=best + 1 if best >= 0 else -1,
                     reference_frame_id=names[b][max(best, 0)] if names[b] else None, **empty(flt, ops.MATCH_RESULT_KEYS))
            if do_covisibility_opt:
                r["refinement"] = None
            out.append(r)
            continue
        p = b * n_db + kept
        n, n_inl = int(rb["count"][p]), int(rb["num_inliers"][p])
        r.update(qvec=rb["qvec"][p].copy(), tvec=rb["tvec"][p].copy(), num_inliers=n_inl, order=kept + 1, reference_frame_id=names[b][kept],
                 **solved(flt, est, order, p, n, n_inl, ops.MATCH_RESULT_KEYS))
        if do_covisibility_opt:
            n2, inl2, ok2 = int(rb["count2"][b]), int(rb["num_inliers2"][b]), bool(rb["success2"][b])
            n_found = int(rb["n_cov_found"][b])
            cov_names = [store.frame_ids[int(g)] for g in rb["cov_frames"][b, :n_found]]
            x = {"success": ok2, "covisible_frame_ids": cov_names, "slots": slot_list(host2, m2, flt2["count"], cov_names, b, n_found, n_cov)}
            x.update({key: stack2[key][b, :n2] for key in _MATCHED})
            if ok2:
                x.update(qvec=rb["qvec2"][b].copy(), tvec=rb["tvec2"][b].copy(), num_inliers=inl2, inliers=est2["inliers"][b, :n2].bool())
                sel = order2[b, :inl2]
                r.update(qvec=x["qvec"], tvec=x["tvec"], num_inliers=inl2, keypoints_query=stack2["matched_keypoints"][b][sel],
                         points3D_ids=stack2["matched_point3D_ids"][b][sel])
            else:      # :351-363: the first pose stays, with no inliers
                x.update(qvec=r["qvec"], tvec=r["tvec"], num_inliers=0, inliers=torch.zeros(n2, dtype=torch.bool, device=dev))
                r.update(num_inliers=0, keypoints_query=r["keypoints_query"][:0], points3D_ids=r["points3D_ids"][:0])
            r["refinement"] = x
        out.append(r)
    return out
