"""Several maps behind one reference store: the tables of MultiMap3D (localization/multimap3d.py:58-93, 119-145) on the device.

The reference keeps one SingleMap3D per scene; sid_scene_name[sid] picks the sub-map of a voted landmark and scene_name_start_sid
its in-map id, and refinement and tracking then run inside sub_maps[matched_scene_name].  MultiMapStore composes already-built
ReferenceStores into ONE store with ReferenceStore's interface, so every stage (candidates, pose, refine, tracker) takes it as it
is: rows, frames, histograms, point lists and covisibility lists are concatenated in map order with their offsets applied, the
landmark tables are laid out by the GLOBAL landmark id with lm_start naming the owning map's start_sid (pram_cand_plan_maps reads
them), and point ids are scoped per map."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from pram_amd.localization.candidates import ReferenceStore, StoreBase

POINT_ID_BITS = 40      # a store point id = map index << 40 | raw id (COLMAP numbers the points of every model from 1)
_RAW_MASK = (1 << POINT_ID_BITS) - 1


class MultiMapStore(StoreBase):
    """maps: ReferenceStores, each built with the start_sid it has in the recogniser's numbering (the reference passes the running
    class count, multimap3d.py:84-90); names: one scene name per map (the reference's matched_scene_name).

    Frames, rows and landmark tables.  Map m's rows follow map m - 1's; store frame index = map_frame_off[m] + in-map index.
    frame_off, sel_rows and lm_sel_off are shifted by the map's row offset, hist_off by its histogram-entry offset, lm_frame,
    pt_frames and covis_frames by its frame offset; hist_label and keypoint_segs stay IN-MAP labels; frame_norm, frame_size, is_vrf,
    covis_off / covis_count are concatenated (the covisibility lists are the maps' own, not recomputed).  lm_frame, lm_sel_off,
    lm_sel_len and lm_start have one entry per global landmark id up to max(start_sid + n_landmarks): entry start_sid_m + l is map
    m's entry l and lm_start is start_sid_m; an id no map owns has lm_frame -1.  The store's own start_sid is 0.

    Point ids.  Inside the store a point id is map index << 40 | raw id, and -1 stays -1: point3D_ids, pt_ids and the keys of the
    per-point tables carry these store ids, and so does every list a stage hands on (matched_point3D_ids, the tracker's state).
    The encoding is monotone in (map, raw id), so pt_ids stays sorted.  split_point_ids / store_point_ids convert.

    Frame ids.  frame_ids[g] = (names[m], the map's own frame id): what the stages report as reference_frame_id."""

    def __init__(self, maps: Sequence[ReferenceStore], names: Sequence[str], device=None):
        maps, names = list(maps), list(names)
        if not maps:
            raise ValueError("MultiMapStore: no map")
        if len(names) != len(maps) or len(set(names)) != len(names):
            raise ValueError("MultiMapStore: needs one unique name per map")
        if len({m.covisibility_frame for m in maps}) != 1:
            raise ValueError("MultiMapStore: the maps differ in covisibility_frame")
        if len(maps) >= 1 << (63 - POINT_ID_BITS):
            raise ValueError("MultiMapStore: too many maps for the point id encoding")
        ranges = sorted((m.start_sid, m.start_sid + len(m.lm_frame), n) for m, n in zip(maps, names) if len(m.lm_frame))
        for (a0, a1, an), (b0, b1, bn) in zip(ranges, ranges[1:]):
            if b0 < a1:
                raise ValueError(f"MultiMapStore: the landmark ranges of {an!r} [{a0}, {a1}) and {bn!r} [{b0}, {b1}) overlap")
        if any(m.start_sid < 0 for m in maps):
            raise ValueError("MultiMapStore: start_sid < 0")
        for m, n in zip(maps, names):
            for ids in (m.point3D_ids, m.pt_ids):
                if ids.size and (int(ids.min()) < -1 or int(ids.max()) > _RAW_MASK):
                    raise ValueError(f"MultiMapStore: map {n!r} has a point id < -1 or >= 2**{POINT_ID_BITS}")
        self.maps, self.names, self.n_maps = maps, names, len(maps)
        self.start_sid = 0
        self.covisibility_frame = maps[0].covisibility_frame
        off = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.map_frame_off = off([m.n_frames for m in maps])
        self.map_row_off = off([m.n_rows for m in maps])
        self.map_point_off = off([len(m.pt_ids) for m in maps])
        hist, ent, cov = off([len(m.hist_label) for m in maps]), off([len(m.pt_frames) for m in maps]), off([len(m.covis_frames) for m in maps])
        for total in (self.map_row_off[-1], hist[-1], ent[-1], cov[-1]):
            if total >= 2 ** 31:
                raise ValueError("MultiMapStore: the concatenated tables do not fit 32-bit offsets")
        cat = lambda name, shift=None: np.concatenate([getattr(m, name) if shift is None else (getattr(m, name) + shift[i]).astype(getattr(m, name).dtype)
                                                       for i, m in enumerate(maps)])
        csr = lambda name, shift: np.concatenate([getattr(maps[0], name)[:1]] + [(getattr(m, name)[1:] + shift[i]).astype(np.int32) for i, m in enumerate(maps)])
        for name in ("keypoints", "scores", "descriptors", "xyzs", "keypoint_segs", "frame_size", "frame_norm", "is_vrf", "hist_label", "hist_cnt",
                     "covis_count"):
            setattr(self, name, cat(name))
        self.point3D_ids = np.concatenate([self.store_point_ids(i, m.point3D_ids) for i, m in enumerate(maps)])
        self.pt_ids = np.concatenate([self.store_point_ids(i, m.pt_ids) for i, m in enumerate(maps)])
        self.frame_off, self.hist_off = csr("frame_off", self.map_row_off), csr("hist_off", hist)
        self.pt_off, self.covis_off = csr("pt_off", ent), csr("covis_off", cov)
        self.sel_rows = cat("sel_rows", self.map_row_off)
        self.pt_frames, self.covis_frames = cat("pt_frames", self.map_frame_off), cat("covis_frames", self.map_frame_off)
        n_lm = max(m.start_sid + len(m.lm_frame) for m in maps)
        self.lm_frame = np.full(n_lm, -1, dtype=np.int32)
        self.lm_sel_off, self.lm_sel_len, self.lm_start = (np.zeros(n_lm, dtype=np.int32) for _ in range(3))
        for i, m in enumerate(maps):
            s = slice(m.start_sid, m.start_sid + len(m.lm_frame))
            self.lm_frame[s] = np.where(m.lm_frame >= 0, m.lm_frame + self.map_frame_off[i], -1)
            self.lm_sel_off[s] = m.lm_sel_off + self.map_row_off[i]
            self.lm_sel_len[s] = m.lm_sel_len
            self.lm_start[s] = m.start_sid
        self.frame_map = np.repeat(np.arange(self.n_maps, dtype=np.int32), [m.n_frames for m in maps])
        self.frame_ids = [(n, fid) for m, n in zip(maps, names) for fid in m.frame_ids]
        self._slices = [{l: (o + int(self.map_row_off[i]), c) for l, (o, c) in sl.items()} for i, m in enumerate(maps) for sl in m._slices]
        self._ready(device)

    # ---- point ids
    @staticmethod
    def store_point_ids(map_index, raw_ids):
        """raw (in-map) point ids of map `map_index` (an int, or an array like raw_ids) -> store ids; -1 stays -1.  numpy or torch."""
        if torch.is_tensor(raw_ids):
            raw = raw_ids.to(torch.int64)
            m = map_index.to(torch.int64) if torch.is_tensor(map_index) else int(map_index)
            return torch.where(raw < 0, raw, raw | (m << POINT_ID_BITS))
        raw = np.asarray(raw_ids, dtype=np.int64)
        return np.where(raw < 0, raw, raw | (np.asarray(map_index, dtype=np.int64) << POINT_ID_BITS))

    @staticmethod
    def split_point_ids(ids):
        """store ids -> (map index, raw id); -1 -> (-1, -1).  numpy or torch."""
        if torch.is_tensor(ids):
            ids = ids.to(torch.int64)
            return torch.where(ids < 0, ids, ids >> POINT_ID_BITS), torch.where(ids < 0, ids, ids & _RAW_MASK)
        ids = np.asarray(ids, dtype=np.int64)
        return np.where(ids < 0, ids, ids >> POINT_ID_BITS), np.where(ids < 0, ids, ids & _RAW_MASK)

    # ---- what the base asks for: lm_start (uploaded and padded like the other landmark tables) and n_maps join tables(); the
    # per-point values are concatenated on first use, each map checking its own then (ReferenceStore's rule)
    _EXTRA_PADDED, _EXTRA_COUNTS = ("lm_start",), ("n_maps",)

    def _point_values(self) -> dict:
        if self._pt_values is None:
            self._pt_values = {name: np.concatenate([getattr(m, name) for m in self.maps]) for name in self._POINT_TABLES}
        return self._pt_values

    def scene_of(self, frame: int) -> str:
        """The name of the map that holds store frame `frame` (the reference's matched_scene_name)."""
        return self.names[int(self.frame_map[frame])]
