"""CPU: the numpy restatement of the reference's map compression (tests/compress_ref.py) against the fixture pinned by running
the reference (tests/golden/compress_pinned.npz, tests/tools/gen_compress_pinned.py), what the scene is made for, and the host side
of pram_amd.localization.compress that needs no GPU."""
from pathlib import Path

import numpy as np
import pytest

from tests import compress_ref as CR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pram_compress_workspace_bytes", "pram_compress_select", "pram_compress_sparsify", "pram_compress_rows")


def test_symbols_declared_and_exported(hip_lib):
    # the entries' declarations, types and exports and header == ops for the constants: tests/test_abi_contract_cpu.py
    from pram_amd import _lib, ops
    assert set(ENTRIES) <= set(_lib.exported_symbols())
    assert CR.ROW_TILE == ops.COMPRESS_ROW_TILE and CR.KPT_TILE == ops.COMPRESS_KPT_TILE
    assert (ROOT / "pram_amd" / "csrc" / "compress.hip").exists()
    assert hip_lib.pram_compress_workspace_bytes(100, 5) == 24 * 100 + 4 * 6 + 16 and hip_lib.pram_compress_workspace_bytes(-1, 5) == 0


def test_scene_is_what_it_is_for():
    s = CR.scene()
    CR.check_scene(s)
    assert CR.vrf_order(s["seg_ref"], 1) == [0, 8, 2, 1]      # frame 0 named twice
    t = s["results"]["c30"]["trace"]
    assert (0, CR.FRAME_LOSER) in t["lost_all"] and CR.FRAME_LOSER not in s["results"]["c30"]["frames"]


@pytest.mark.parametrize("tag", list(CR.CONFIGS))
def test_restatement_reproduces_the_reference(golden, tag):
    """Frames and their order, every frame's list, every point's frame list and the points' order: exact."""
    g, r = golden("compress_pinned"), CR.scene()["results"][tag]
    assert int(g["seed"]) == CR.SEED
    assert g[tag + "_frames"].tolist() == r["frames"]
    off, ids = g[tag + "_list_off"], g[tag + "_list_ids"]
    for i, f in enumerate(r["frames"]):
        assert np.array_equal(ids[off[i]:off[i + 1]], r["lists"][f]), (tag, f)
    assert g[tag + "_pt_ids"].tolist() == list(r["point_frames"])
    off, frames = g[tag + "_pt_off"], g[tag + "_pt_frames"]
    for i, p in enumerate(g[tag + "_pt_ids"].tolist()):
        assert frames[off[i]:off[i + 1]].tolist() == r["point_frames"][p], (tag, p)
    if CR.CONFIGS[tag]["nkpts"] > 0:
        assert max(len(r["lists"][f]) for f in r["trace"]["sparsified"]) > CR.CONFIGS[tag]["nkpts"]      # the cap is no cap: one per cell


def test_projected_keypoints_against_the_reference(golden):
    """associate_keypoints_with_point3Ds: the projections within 1e-9 px of the reference's matrix products, the scores exactly."""
    g, s = golden("compress_pinned"), CR.scene()
    for f in g["assoc_frames"].tolist():
        ids, ref = g[f"assoc_{f}_ids"], g[f"assoc_{f}_keypoints"]
        assert np.array_equal(ids, s["results"]["c30"]["lists"][f])
        mine = CR.frame_rows(s, f, ids)["keypoints"]
        assert np.abs(mine[:, :2] - ref[:, :2]).max() <= 1e-9
        assert np.array_equal(mine[:, 2], ref[:, 2])
    err = s["pt_err"]
    assert (err * 5 < 1).any() and (err * 5 > 20).any()      # both ends of the clip


def test_sparsify_restatement_rules():
    cam = np.array([1.0, 0, 0, 0, 0, 0, 0, 512.0, 512.0, 0, 0, 640, 480])
    px = lambda u, v: [u / 512.0, v / 512.0, 1.0]
    xyz = np.array([px(5, 5), px(45, 5), px(6, 6), px(40.0, 30), px(-3, 7), px(7, 7)])
    win, _ = CR.sparsify(cam, xyz, np.array([3, 1, 3, 2, 9, 4]), 20.0)
    # cell (0, 0): positions 0, 2 tie at 3 (the earlier holds), then 5 beats them; 45 and 40.0 share cell 2 of row 0 / row 1; -3 is cell -1
    assert win.tolist() == [5, 1, 3, 4]
    assert np.rint(np.float64(40.0) // 20.0) == 2 and np.rint(np.float64(-3.0) // 20.0) == -1


def test_vrf_order_and_argument_checks():
    from pram_amd._lib import PramHipError
    from pram_amd.localization import compress as CP
    from pram_amd.localization.candidates import ReferenceStore
    assert CP.vrf_order({3: [7, 8], 1: [9], 2: [7, 5], 4: []}, 1) == [7, 9]
    assert CP.vrf_order({3: [7, 8], 1: [9], 2: [7, 5]}, 2) == [7, 8, 9, 5]
    assert CP.vrf_order([[4, 2], [4], [1]]) == [4, 1]
    with pytest.raises(ValueError):
        CP.vrf_order({0: [1]}, 0)
    s = CR.scene()
    store = ReferenceStore(CR.store_frames(s), **CR.store_arguments(s, 5))
    for f in CR.vrf_order(s["seg_ref"], 1):      # the store's graph is the restatement's candidate order
        want = CR.covisible_lists(s["frame_off"], s["point3D_ids"], s["point_frames"], [f], 5)[f][0]
        assert store.covisible(f).tolist() == want
    ids = [CR.FRAME_ID0 + f for f in CR.vrf_order(s["seg_ref"], 1)]
    ok = dict(radius=20, xys=s["xys"], device="cpu")
    with pytest.raises(ValueError, match="cams"):
        CP.compress_map(store, s["cams"][:3], ids, **ok)
    with pytest.raises(ValueError, match="not in the store"):
        CP.compress_map(store, s["cams"], [999], **ok)
    with pytest.raises(ValueError, match="no covisible list"):
        CP.compress_map(store, s["cams"], [CR.FRAME_ID0 + 6], **ok)      # frame 6 is no landmark's frame
    with pytest.raises(ValueError, match="radius"):
        CP.compress_map(store, s["cams"], ids, radius=0, device="cpu")
    with pytest.raises(ValueError, match="xys"):
        CP.compress_map(store, s["cams"], ids, xys=s["xys"][:-1], device="cpu")
    with pytest.raises(ValueError, match="point3D_obs"):
        CP.compress_map(store, s["cams"], ids, nkpts=10, point3D_obs=np.zeros(3), device="cpu")
    with pytest.raises(PramHipError):      # every argument in order: only the device is wrong
        CP.compress_map(store, s["cams"], ids, **ok)
    with pytest.raises(ValueError, match="point3D_errors"):
        CP.project_rows(store, s["cams"], [0], [0], {1: 0.5}, "cpu")
    assert "recmap.py:668-922" in CP.__doc__ and "count descending, frame index ascending" in CP.__doc__
    # frame_lists: the compressed lists, a reference frame's list replaced and cut to the points the compressed map holds
    r = s["results"]["c30"]
    result = {"frame_ids": [CR.FRAME_ID0 + f for f in r["frames"]], "frame_point_ids": {CR.FRAME_ID0 + f: v for f, v in r["lists"].items()},
              "point_ids": np.array(list(r["point_frames"]), dtype=np.int64)}
    held = result["point_ids"]
    gone = np.setdiff1d(s["pt_ids"], held)
    assert len(gone)
    fids, row_frame, row_point, counts = CP.frame_lists(store, result, {CR.FRAME_ID0 + 8: [int(held[3]), int(gone[0]), int(held[0])], CR.FRAME_ID0 + 4: [int(gone[0])]})
    assert fids == [x for x in result["frame_ids"] if x != CR.FRAME_ID0 + 4] and counts[fids.index(CR.FRAME_ID0 + 8)] == 2
    a = int(np.sum(counts[:fids.index(CR.FRAME_ID0 + 8)]))
    assert store.pt_ids[row_point[a:a + 2]].tolist() == [int(held[3]), int(held[0])] and row_frame[a:a + 2].tolist() == [8, 8]
