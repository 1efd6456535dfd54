"""GPU: map building on the device (pram_amd.localization.mapbuild, csrc/mapbuild.hip) against the numpy restatement
tests/mapbuild_ref.py on its shared scene: the point descriptors on every track, the virtual reference frames of the 8 landmarks
(which landmark takes which branch: tests/mapbuild_ref.py LM_* and tests/test_mapbuild_cpu.py), the way into a ReferenceStore, and
the C entries' refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mapbuild_ref as MR

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-12      # the float64 rounding of a 128-term dot of unit vectors is ~3e-14: medians closer than this may go either way


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def run(dev):
    """Both stages once (and once more, for determinism) on the scene's own CSR tables, which hold frame indices out of range."""
    from pram_amd.localization import mapbuild as MB
    from pram_amd.localization.candidates import ReferenceStore
    s = MR.scene()
    store = ReferenceStore(s["frames"], {}, point3D_frame_ids={p: v[0] for p, v in s["tracks"].items()})
    assert np.array_equal(store.pt_ids, s["point_ids"])
    tables = {k: s[k] for k in ("point_ids", "trk_off", "trk_frame", "trk_kpt")}
    pt_xyz = np.array([s["xyz"][p] for p in store.pt_ids.tolist()])
    out = {"scene": s, "store": store, "tables": tables, "pt_xyz": pt_xyz}
    for tag in ("", "_again"):
        d, c = MB.assign_point_descriptors(store, tables, dev)
        out["desc" + tag], out["choice" + tag] = d.cpu().numpy(), c.cpu().numpy()
        out["vrf" + tag], out["vrf_n" + tag] = MB.select_reference_frames(store, s["landmarks"], s["cams"], pt_xyz, dev, s["ignored"], **MR.VRF_PARAMS)
    return out


def _at(s, name):
    return s["index_of_point"][s["special"][name]]


def test_choices_equal_the_restatement(run):
    s, got = run["scene"], run["choice"]
    assert got.shape == s["choice"].shape and got.dtype == np.int32
    near = 0
    for i in np.nonzero(got != s["choice"])[0].tolist():
        pos, med = s["medians"][i]
        assert got[i] in pos.tolist(), (i, got[i])
        a, b = med[pos.tolist().index(got[i])], med[pos.tolist().index(s["choice"][i])]
        print(f"point {s['point_ids'][i]}: device {got[i]} (median {a!r}), restatement {s['choice'][i]} (median {b!r})")
        assert a != b and abs(a - b) <= NEAR_TIE, i      # bit-equal medians are a tie: the lowest position, as the restatement
        near += 1
    assert near <= 0.01 * len(got), near


def test_descriptor_is_a_bit_copy_of_the_chosen_row(run):
    s, got, choice = run["scene"], run["desc"], run["choice"]
    rows = MR.entry_rows(s["frame_off"].astype(np.int64), s["trk_frame"], s["trk_kpt"])
    want = np.zeros_like(got)
    for i in range(len(choice)):
        if choice[i] >= 0:
            r = rows[s["trk_off"][i] + choice[i]]
            assert r >= 0, i
            want[i] = s["descriptors"][r]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_named_tracks(run):
    s, choice, desc = run["scene"], run["choice"], run["desc"]
    assert choice[_at(s, "all_dropped")] == -1 and not desc[_at(s, "all_dropped")].view(np.uint32).any()
    assert choice[_at(s, "one_kept")] == 1 == s["choice"][_at(s, "one_kept")]
    for name in ("dropped_short", "dropped_long"):      # dropped entries: -1 frames, frames out of range, keypoints outside the frame
        i = _at(s, name)
        assert choice[i] == s["choice"][i] and choice[i] in s["medians"][i][0].tolist(), name
    assert s["medians"][_at(s, "dropped_short")][0].tolist() == [0, 2]
    for name in ("repeat_0_k", "repeat_k_last", "repeat_all", "repeat_long"):      # a bit-identical row repeated
        assert choice[_at(s, name)] == s["choice"][_at(s, name)], name
    assert choice[_at(s, "repeat_all")] == 0
    # every path: one wave's worth in LDS, the Gram row in LDS, the Gram row in the workspace, and both sides of each boundary
    for n in (1, 2, 3, 4, 5, 8, 17, 63, 64, 65, 130, 300, MR.SHORT - 1, MR.SHORT, MR.SHORT + 1, MR.ROW_LDS - 1, MR.ROW_LDS, MR.ROW_LDS + 1):
        assert choice[_at(s, f"len{n}")] == s["choice"][_at(s, f"len{n}")], n


def test_two_runs_are_bit_equal(run):
    assert np.array_equal(run["choice"], run["choice_again"]) and np.array_equal(run["desc"].view(np.uint32), run["desc_again"].view(np.uint32))
    assert np.array_equal(run["vrf"], run["vrf_again"]) and np.array_equal(run["vrf_n"], run["vrf_n_again"])


def test_reference_frames_equal_the_restatement(run):
    s, vrf, n = run["scene"], run["vrf"], run["vrf_n"]
    assert vrf.shape == (8, MR.VRF_PARAMS["n_vrf"]) and n.shape == (8,)
    for sid, want in enumerate(s["vrf"]):
        assert vrf[sid, :n[sid]].tolist() == want and (vrf[sid, n[sid]:] == -1).all(), (sid, vrf[sid], want)


def test_build_store_inputs_feeds_a_reference_store(run, dev):
    from pram_amd.localization import mapbuild as MB
    from pram_amd.localization.candidates import ReferenceStore
    s = run["scene"]
    out = MB.build_store_inputs(s["frames"], s["tracks"], dict(enumerate(s["landmarks"])), s["xyz"], dev, s["ignored"], **MR.VRF_PARAMS)
    sids = {int(p): 0 for p in s["point_ids"].tolist()}      # the labels come from the clustering, which is not part of this
    store = ReferenceStore(s["frames"], point3D_sids=sids, **{k: out[k] for k in MB.STORE_KEYS})
    assert np.array_equal(store.pt_ids, s["point_ids"])
    assert np.array_equal(store.pt_desc.view(np.uint32), run["desc"].view(np.uint32))
    assert [out["point3D_choice"][p] for p in s["point_ids"].tolist()] == run["choice"].tolist()
    first = [v[0] if v else -1 for v in s["vrf"]]
    assert store.lm_frame.tolist() == first
    assert out["seg_ref_frame_ids"] == {sid: [MR.FRAME_ID0 + f for f in v] for sid, v in enumerate(s["vrf"])}


def test_c_entries_refuse_without_launching(run, dev, hip_lib):
    """A null pointer, a misaligned descriptor buffer and a workspace that is too small: PRAM_E_ARG, and the outputs untouched."""
    L, s, t = hip_lib, run["scene"], run["store"].tables(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P = len(s["point_ids"])
    off_host = (C.c_int * (P + 1))(*s["trk_off"].tolist())
    trk_off, trk_frame, trk_kpt = up(s["trk_off"]), up(s["trk_frame"]), up(s["trk_kpt"])
    need = L.pram_mapbuild_desc_workspace_bytes(C.addressof(off_host), P)
    assert need == 12 * int(max(s["trk_off"][i + 1] for i in range(P) if s["trk_off"][i + 1] - s["trk_off"][i] > MR.SHORT))
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    pt_desc = torch.full((P, 128), 7.0, device=dev)
    pt_choice = torch.full((P,), -77, device=dev, dtype=torch.int32)
    desc_pad = torch.zeros(t["descriptors"].numel() + 4, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def assign(descriptors=t["descriptors"].data_ptr(), workspace_bytes=need, out=pt_desc.data_ptr()):
        return L.pram_mapbuild_assign_descriptors(descriptors, t["frame_off"].data_ptr(), t["n_frames"], t["n_rows"], trk_off.data_ptr(),
                                                  C.addressof(off_host), trk_frame.data_ptr(), trk_kpt.data_ptr(), P, ws.data_ptr(), workspace_bytes,
                                                  out, pt_choice.data_ptr(), st)
    assert assign(descriptors=None) == -1 and b"null" in L.pram_last_error()
    assert assign(out=None) == -1
    assert assign(descriptors=desc_pad.data_ptr() + 4) == -1 and b"16-byte" in L.pram_last_error()
    assert assign(workspace_bytes=need - 1) == -1 and b"workspace" in L.pram_last_error()
    torch.cuda.synchronize()
    assert (pt_choice == -77).all() and (pt_desc == 7.0).all()

    lm_off_np, lm_pts = np.zeros(9, dtype=np.int32), np.concatenate([np.asarray(v, dtype=np.int64) for v in s["landmarks"] if len(v)])
    lm_off_np[1:] = np.cumsum([len(v) for v in s["landmarks"]])
    lm_host = (C.c_int * 9)(*lm_off_np.tolist())
    lm_off, lm_points, ignored, cams, pt_xyz = up(lm_off_np), up(lm_pts), up(s["ignored"]), up(s["cams"]), up(run["pt_xyz"])
    n_vrf = MR.VRF_PARAMS["n_vrf"]
    vneed = L.pram_mapbuild_vrf_workspace_bytes(8, len(lm_pts), t["n_frames"])
    assert vneed > 0
    vws = torch.empty(vneed, device=dev, dtype=torch.uint8)
    lm_vrf = torch.full((8, n_vrf), -77, device=dev, dtype=torch.int32)
    lm_vrf_n = torch.full((8,), -77, device=dev, dtype=torch.int32)

    def select(ids=t["point3D_ids"].data_ptr(), workspace_bytes=vneed, xyz=pt_xyz.data_ptr(), n=n_vrf):
        p = MR.VRF_PARAMS
        return L.pram_mapbuild_select_frames(ids, t["frame_off"].data_ptr(), t["n_frames"], t["n_rows"], t["pt_ids"].data_ptr(), t["pt_off"].data_ptr(),
                                             t["pt_frames"].data_ptr(), t["n_points"], t["n_pt_entries"], xyz, lm_off.data_ptr(), C.addressof(lm_host),
                                             lm_points.data_ptr(), 8, ignored.data_ptr(), cams.data_ptr(), p["min_obs"], p["topk_imgs"], n,
                                             p["min_cover_ratio"], p["gain_floor"], vws.data_ptr(), workspace_bytes, lm_vrf.data_ptr(),
                                             lm_vrf_n.data_ptr(), st)
    assert select(ids=None) == -1 and b"null" in L.pram_last_error()
    assert select(xyz=pt_xyz.data_ptr() + 4) == -1 and b"aligned" in L.pram_last_error()
    assert select(workspace_bytes=vneed - 1) == -1 and b"workspace" in L.pram_last_error()
    assert select(n=65) == -1
    torch.cuda.synchronize()
    assert (lm_vrf == -77).all() and (lm_vrf_n == -77).all()
    # and the same calls, complete, succeed
    assert assign() == 0 and select() == 0
    torch.cuda.synchronize()
    assert np.array_equal(pt_choice.cpu().numpy(), run["choice"]) and np.array_equal(lm_vrf_n.cpu().numpy(), run["vrf_n"])
