"""Writes tests/golden/multimap_pinned.npz: what the REFERENCE's MultiMap3D.run (localization/multimap3d.py:95-145) decides per
voted landmark on tests/multimap_ref.py::two_maps with pinned_cases: which sub-map it goes to, with which in-map id, which query
keypoints and whether semantically.

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are); never runs in
the test suite.  The MultiMap3D and its two SingleMap3D sub-maps are built with __new__ and given the tables initialize_map would
fill (sid_scene_name, scene_name_start_sid; start_sid, seg_ref_frame_ids, point3Ds, reference_frames); the reference's own
process_segmentations and check_semantic_consistency run; localize_with_ref_frame is a recorder that keeps what it is handed and
answers success False, so the loop visits every candidate.  The fixture holds results only; the scene regenerates from its seeds.

    python tests/tools/gen_multimap_pinned.py
"""
from __future__ import annotations

import contextlib
import io
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import gen_golden as G  # noqa: E402
from tests import multimap_ref as MR  # noqa: E402


def main():
    G.import_reference()
    G._stub_missing_modules()
    import localization.multimap3d as ref_mm
    import localization.singlemap3d as ref_sm
    maps = MR.two_maps()
    mm = ref_mm.MultiMap3D.__new__(ref_mm.MultiMap3D)
    mm.sid_scene_name, mm.scene_name_start_sid, mm.sub_maps = [], {}, {}
    mm.loc_config = {"show": False, "seg_k": MR.TWO_SEG_K, "min_kpts": MR.TWO_MIN_KPTS}
    mm.do_refinement, mm.semantic_matching = False, True
    calls = []
    for name, m in zip(MR.TWO_NAMES, maps):
        sm = ref_sm.SingleMap3D.__new__(ref_sm.SingleMap3D)
        sm.start_sid, sm.image_path_prefix = m["start_sid"], ""
        sm.seg_ref_frame_ids = {l: np.array(v) for l, v in m["seg_ref_frame_ids"].items()}
        sm.point3Ds = {int(pid): SimpleNamespace(seg_id=int(s)) for f in m["frames"] for pid, s in zip(f["point3D_ids"], f["keypoint_segs"])}
        sm.reference_frames = {f["id"]: SimpleNamespace(point3D_ids=f["point3D_ids"]) for f in m["frames"]}

        def localize(q_frame, q_kpt_ids, sid, semantic_matching, name=name):
            calls.append((name, int(sid), np.asarray(q_kpt_ids).astype(np.int64), bool(semantic_matching)))
            return {"success": False, "matched_keypoints": np.zeros((0, 2), np.float32), "num_inliers": 0}
        sm.localize_with_ref_frame = localize
        mm.sub_maps[name] = sm
        # initialize_map, multimap3d.py:87-90 (the running class count is the map's start_sid)
        assert len(mm.sid_scene_name) == m["start_sid"]
        mm.sid_scene_name = mm.sid_scene_name + [name for _ in range(MR.n_landmarks(m))]
        mm.scene_name_start_sid[name] = m["start_sid"]
    out = {"seg_k": MR.TWO_SEG_K, "min_kpts": MR.TWO_MIN_KPTS, "names": np.array(MR.TWO_NAMES)}
    seen = set()
    cases = MR.pinned_cases(maps)
    for b, q in enumerate(cases):
        q = MR.real(q)
        q_frame = SimpleNamespace(segmentations=q["segmentations"], seg_ids=q["seg_ids"], keypoints=q["keypoints"], scene_name="s", name=f"q{b}",
                                  time_loc=0.0, tracking_status=None)
        calls.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            assert mm.run(q_frame) is False
        assert len(calls) == MR.TWO_SEG_K
        out[f"q{b}_scene"] = np.array([MR.TWO_NAMES.index(c[0]) for c in calls], dtype=np.int32)
        out[f"q{b}_lsid"] = np.array([c[1] for c in calls], dtype=np.int32)
        out[f"q{b}_semantic"] = np.array([c[3] for c in calls], dtype=np.int32)
        for w, c in enumerate(calls):
            out[f"q{b}_c{w}_kpt_ids"] = c[2]
            seen.add((c[0], c[3]))
            if c[0] == MR.TWO_NAMES[1] and c[1] == 0:
                seen.add("second_map_sid0")
        if len({c[0] for c in calls[:2]}) == 2:
            seen.add("both_maps")
        print(f"  query {b}: " + ", ".join(f"{c[0]}/{c[1]}{'*' if c[3] else ''}({len(c[2])})" for c in calls))
    want = {(n, s) for n in MR.TWO_NAMES for s in (False, True)} | {"second_map_sid0", "both_maps"}
    assert seen == want, seen
    out["n_queries"] = len(cases)
    G.save("multimap_pinned", **out)


if __name__ == "__main__":
    main()
