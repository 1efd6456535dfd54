"""CPU: the numpy restatement of the reference's map-building stages (tests/mapbuild_ref.py) against the fixture pinned by running
the reference (tests/golden/mapbuild_pinned.npz, tests/tools/gen_mapbuild_pinned.py), the branches the scene's landmarks take, and
the host side of pram_amd.localization.mapbuild that needs no GPU."""
from pathlib import Path

import numpy as np
import pytest

from tests import mapbuild_ref as MR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_mapbuild_desc_workspace_bytes", "pram_mapbuild_assign_descriptors", "pram_mapbuild_vrf_workspace_bytes",
           "pram_mapbuild_select_frames")
# A 128-term fp32 dot of unit vectors errs by at most 128 * 2^-24 = 7.6e-6, a distance 2 - 2 dot by twice that, a difference of
# two medians by at most ~3e-5: the reference's fp32 choice is only pinned where the float64 medians are further apart than this.
GAP = 4e-5


def test_symbols_declared_and_exported(hip_lib):
    # the entries' declarations, types and exports and header == ops for the constants: tests/test_abi_contract_cpu.py
    from pram_amd import _lib, ops
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    assert MR.SHORT == ops.MAPBUILD_SHORT_TRACK and MR.ROW_LDS == ops.MAPBUILD_ROW_LDS
    assert (ROOT / "pram_amd" / "csrc" / "mapbuild.hip").exists()


def test_vrf_restatement_reproduces_the_reference(golden):
    g, s = golden("mapbuild_pinned"), MR.scene()
    assert int(g["seed"]) == MR.SEED and g["vrf"].shape == (8, MR.VRF_PARAMS["n_vrf"])
    for sid, want in enumerate(s["vrf"]):
        assert g["vrf"][sid, :g["vrf_n"][sid]].tolist() == want and (g["vrf"][sid, g["vrf_n"][sid]:] == -1).all(), sid


def test_scene_landmarks_take_every_branch():
    """Which landmark takes which branch of recmap.py:263-403, from the restatement's trace."""
    t = MR.scene()["traces"]
    a = t[MR.LM_COUNT_GAIN_TIES_COVERAGE]
    assert a["count_tie"] and a["gain_tie"] and a["stop"] == "coverage" and a["chosen"] == [2, 0]      # encounter order 2, 0, 1 decides both ties
    a = t[MR.LM_FALLBACK_NONE_LEFT]
    assert a["fallback"] and a["stop"] == "none left" and a["chosen"] == [9, 8]
    a = t[MR.LM_TOPK_CUT_NVRF]
    assert a["topk_cut"] and a["count_tie"] and a["stop"] == "n_vrf" and 5 not in a["chosen"]      # frame 5 sees every point and is cut
    a = t[MR.LM_ZERO_GAIN_FLOOR]
    assert a["zero_gain"] and a["stop"] == "gain floor" and a["chosen"] == [4, 5]
    a = t[MR.LM_IGNORED_ID0_LACKING_REPEATED]
    assert a["ignored"] and a["id0"] and a["lacking"] and a["repeated"] and a["stop"] == "none left" and MR.IGNORED_FRAME not in a["chosen"]
    a = t[MR.LM_DROP7]
    assert a["drop7"] and not a["drop8"] and a["stop"] == "coverage" and a["chosen"] == [3, 2] and MR.scene()["vrf"][MR.LM_DROP7] == [3]
    a = t[MR.LM_DROP8]
    assert a["drop8"] and not a["drop7"] and a["chosen"] == [MR.OUTSIDE_FRAME, MR.ZERO_Z_FRAME, 0] and MR.scene()["vrf"][MR.LM_DROP8] == [0]
    assert MR.scene()["landmarks"][MR.LM_EMPTY] == [] and MR.scene()["vrf"][MR.LM_EMPTY] == []
    assert {x["stop"] for x in t if "stop" in x} == {"coverage", "gain floor", "n_vrf", "none left"}


def test_descriptor_pin_through_the_gap(golden):
    """The reference's fp32 BLAS choice against the float64 restatement: always a row within GAP of the smallest median; the same
    row wherever exactly one row lies within GAP; and that must be the common case on tracks of four and more."""
    g, s = golden("mapbuild_pinned"), MR.scene()
    assert len(g["desc_point_ids"]) >= 290
    decided = long_tracks = lowest_of_tie = short_tracks = 0
    for p, ref_choice in zip(g["desc_point_ids"].tolist(), g["desc_choice"].tolist()):
        i = s["index_of_point"][p]
        pos, med = s["medians"][i]
        near = pos[med - med.min() <= GAP]
        assert ref_choice in near.tolist(), (p, ref_choice, near)
        if len(pos) in (2, 3):      # pure ties by construction: the reference chose a tied row, no more is asserted
            short_tracks += 1
            lowest_of_tie += ref_choice == near.min()
            continue
        if len(pos) >= 4:
            long_tracks += 1
        if len(near) == 1:
            assert ref_choice == s["choice"][i], p
            decided += len(pos) >= 4
    assert long_tracks >= 150 and decided >= 0.8 * long_tracks, (decided, long_tracks)
    assert short_tracks >= 10
    print(f"tracks of 2 and 3: the reference chose the lowest tied position on {lowest_of_tie} of {short_tracks}")


def test_restatement_tie_rule_and_drops():
    s = MR.scene()
    at = lambda name: s["index_of_point"][s["special"][name]]
    assert s["choice"][at("all_dropped")] == -1 and not s["desc"][at("all_dropped")].any()
    assert s["choice"][at("one_kept")] == 1 and s["choice"][at("repeat_all")] == 0 and s["choice"][at("len1")] == 0
    assert s["medians"][at("dropped_short")][0].tolist() == [0, 2] and len(s["medians"][at("dropped_long")][0]) == 30
    # a track of three: the two rows of the closest pair tie exactly, and the lower position wins
    pos, med = s["medians"][at("len3")]
    assert np.sort(med)[0] == np.sort(med)[1] and s["choice"][at("len3")] == pos[med == med.min()].min()
    G = MR.gram_batch(s["descriptors"][None, :9])
    assert np.array_equal(G, G.transpose(0, 2, 1))


def test_module_without_a_gpu():
    from pram_amd._lib import PramHipError
    from pram_amd.localization import mapbuild as MB
    from pram_amd.localization.candidates import ReferenceStore
    s = MR.scene()
    store = ReferenceStore(s["frames"], {}, point3D_frame_ids={p: v[0] for p, v in s["tracks"].items()})
    t = MB.track_tables(store, s["tracks"])
    assert np.array_equal(t["point_ids"], s["point_ids"]) and np.array_equal(t["trk_off"], s["trk_off"]) and np.array_equal(t["trk_kpt"], s["trk_kpt"])
    held = (s["trk_frame"] >= 0) & (s["trk_frame"] < MR.F)
    assert np.array_equal(t["trk_frame"], np.where(held, s["trk_frame"], -1))
    assert np.array_equal(MB.frame_cameras(s["frames"]), s["cams"])
    with pytest.raises(PramHipError):
        MB.assign_point_descriptors(store, t, "cpu")
    with pytest.raises(ValueError):
        MB.frame_cameras([{"width": 1, "height": 1}])
    assert "recmap.py:124-194" in MB.__doc__ and "lowest track position" in MB.__doc__
