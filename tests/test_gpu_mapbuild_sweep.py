"""GPU: map building at production shapes (csrc/mapbuild.hip through ops.mapbuild_select_frames and ops.mapbuild_assign_descriptors)
against the numpy restatement on the sweep scenes of tests/mapbuild_ref.py: landmarks of more than 256 points and of whole mask
words, more than 256 frames / eligible frames / candidates, n_vrf = 64, ids beyond 2^32, a probe chain that wraps, ragged and empty
frames, reused and pre-filled workspaces, and tracks whose row indices and Gram row live in the workspace.  Which scene reaches
which path is asserted on the CPU (tests/test_mapbuild_sweep_cpu.py).  Every reference-frame comparison is exact."""
import numpy as np
import pytest
import torch

from tests import mapbuild_ref as MR

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-12      # as tests/test_gpu_mapbuild.py: medians closer than this may go either way


@pytest.fixture(scope="module")
def dev(hip_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _up(a, dev):
    a = np.ascontiguousarray(a)
    if a.shape[0] == 0:      # never an empty allocation behind a pointer
        a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
    return torch.from_numpy(a).to(dev)


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in lists])
    return off, np.array([p for v in lists for p in v], dtype=np.int64)


_uploaded = {}


def _tables(s, dev):
    """The plain dict of device tables ops.mapbuild_select_frames takes, and the call's other arguments (uploaded once)."""
    if id(s) not in _uploaded:
        lm_off, lm_points = _csr(s["landmarks"])
        t = {"point3D_ids": _up(s["point3D_ids"], dev), "frame_off": _up(s["frame_off"], dev), "n_frames": s["F"], "n_rows": len(s["point3D_ids"]),
             "pt_ids": _up(s["pt_ids"], dev), "pt_off": _up(s["pt_off"], dev), "pt_frames": _up(s["pt_frames"], dev), "n_points": len(s["pt_ids"]),
             "n_pt_entries": len(s["pt_frames"])}
        _uploaded[id(s)] = (t, (_up(s["pt_xyz"], dev), _up(lm_off, dev), lm_off, _up(lm_points, dev), _up(s["ignored"], dev), _up(s["cams"], dev)), len(lm_points))
    return _uploaded[id(s)]


def _select(s, dev, workspace=None):
    from pram_amd import ops
    t, args, _ = _tables(s, dev)
    vrf, n = ops.mapbuild_select_frames(t, *args, workspace=workspace, **s["params"])
    return vrf.cpu().numpy(), n.cpu().numpy()


def _need(s, dev, hip_lib):
    t, _, total = _tables(s, dev)
    return int(hip_lib.pram_mapbuild_vrf_workspace_bytes(len(s["landmarks"]), total, s["F"]))


@pytest.mark.parametrize("name", MR.SWEEP_NAMES)
def test_reference_frames_equal_the_restatement(name, dev):
    for tag, s in MR.sweep_calls(name).items():
        vrf, n = _select(s, dev)
        assert vrf.shape == (len(s["landmarks"]), s["params"]["n_vrf"]) and n.shape == (len(s["landmarks"]),) and vrf.dtype == np.int32
        bad = [l for l, want in enumerate(s["vrf"]) if n[l] != len(want) or vrf[l, :len(want)].tolist() != want or not (vrf[l, len(want):] == -1).all()]
        for l in bad:
            print(f"{tag}: landmark {l} of {len(s['landmarks'][l])} points: device {vrf[l].tolist()} (n {n[l]}), restatement {s['vrf'][l]}, trace {s['traces'][l]}")
        assert not bad, (tag, bad)
        vrf2, n2 = _select(s, dev)      # determinism: the bits of a second run
        assert np.array_equal(vrf, vrf2) and np.array_equal(n, n2), tag


def test_workspace_contents_do_not_matter(dev, hip_lib):
    """The sections the host does not set (cand, efr, unobs, fcount, the tail of ekey) hold whatever the buffer held: all ones, zeros,
    0xA5, a larger buffer, and what another scene's call left behind."""
    wide = MR.sweep_scene("wide")
    fresh = _select(wide, dev)
    need = _need(wide, dev, hip_lib)
    assert need > 0
    same = lambda got, want: np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for fill in (0xFF, 0x00, 0xA5):
        assert same(_select(wide, dev, torch.full((need,), fill, device=dev, dtype=torch.uint8)), fresh), hex(fill)
    assert same(_select(wide, dev, torch.full((need + 4096,), 0x5A, device=dev, dtype=torch.uint8)), fresh)
    shared = torch.full((need,), 0xFF, device=dev, dtype=torch.uint8)
    assert same(_select(wide, dev, shared), fresh)
    for tag, s in MR.sweep_calls("degenerate").items():
        assert _need(s, dev, hip_lib) <= need
        assert same(_select(s, dev, shared), _select(s, dev)), tag
    assert same(_select(wide, dev, shared), fresh)
    for l, want in enumerate(wide["vrf"]):
        assert fresh[0][l, :fresh[1][l]].tolist() == want, l


@pytest.fixture(scope="module")
def long_run(dev):
    from pram_amd import ops
    s = MR.long_track_scene()
    store = {"descriptors": _up(s["descriptors"], dev), "frame_off": _up(s["frame_off"], dev), "n_frames": s["n_frames"], "n_rows": s["n_rows"]}
    frame, kpt = _up(s["trk_frame"], dev), _up(s["trk_kpt"], dev)

    def assign(n_points=None, workspace=None):
        off = s["trk_off"] if n_points is None else s["trk_off"][:n_points + 1]
        d, c = ops.mapbuild_assign_descriptors(store, _up(off, dev), off, frame, kpt, workspace=workspace)
        return d.cpu().numpy(), c.cpu().numpy()
    return {"scene": s, "assign": assign, "first": assign(), "again": assign()}


def test_long_tracks_equal_the_restatement(long_run):
    s, (desc, choice) = long_run["scene"], long_run["first"]
    assert choice.shape == s["choice"].shape and choice.dtype == np.int32
    named = {i: k for k, i in s["special"].items()}
    near = 0
    for i in np.nonzero(choice != s["choice"])[0].tolist():
        pos, med = s["medians"][i]
        assert choice[i] in pos.tolist(), (i, named.get(i), choice[i])
        a, b = med[pos.tolist().index(choice[i])], med[pos.tolist().index(s["choice"][i])]
        print(f"track {i} ({named.get(i)}): device {choice[i]} (median {a!r}), restatement {s['choice'][i]} (median {b!r})")
        assert a != b and abs(a - b) <= NEAR_TIE, (i, named.get(i))      # bit-equal medians are a tie: the lowest position
        near += 1
    assert near <= 1, near
    # the descriptor is a bit copy of the chosen row
    rows = MR.entry_rows(s["frame_off"].astype(np.int64), s["trk_frame"], s["trk_kpt"])
    want = np.zeros_like(desc)
    for i in range(len(choice)):
        assert choice[i] >= 0 and rows[s["trk_off"][i] + choice[i]] >= 0, i
        want[i] = s["descriptors"][rows[s["trk_off"][i] + choice[i]]]
    assert np.array_equal(desc.view(np.uint32), want.view(np.uint32))
    i = s["special"]["repeat_long"]
    assert choice[i] == s["choice"][i]


def test_long_tracks_workspace_and_determinism(long_run, hip_lib, dev):
    import ctypes as C
    s, (desc, choice) = long_run["scene"], long_run["first"]
    assert np.array_equal(choice, long_run["again"][1]) and np.array_equal(desc.view(np.uint32), long_run["again"][0].view(np.uint32))
    P = len(s["trk_off"]) - 1
    host = (C.c_int * (P + 1))(*s["trk_off"].tolist())
    need = int(hip_lib.pram_mapbuild_desc_workspace_bytes(C.addressof(host), P))
    assert need == 12 * int(s["trk_off"][s["n_prefix"]]) < 12 * int(s["trk_off"][P])      # short tracks beyond the workspace's end
    # all ones read as float64 is NaN, the kernel's own mark of a dropped entry
    d, c = long_run["assign"](workspace=torch.full((need,), 0xFF, device=dev, dtype=torch.uint8))
    assert np.array_equal(c, choice) and np.array_equal(d.view(np.uint32), desc.view(np.uint32))
    # cut after the last long track: the workspace ends with the entries
    P1 = s["n_prefix"]
    d, c = long_run["assign"](n_points=P1)
    assert np.array_equal(c, choice[:P1]) and np.array_equal(d.view(np.uint32), desc[:P1].view(np.uint32))
