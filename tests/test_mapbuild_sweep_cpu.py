"""CPU: the sweep scenes of tests/mapbuild_ref.py reach the shape classes of csrc/mapbuild.hip they are built for (asserted from the
restatement's traces, so that the reference alone proves it), the restatement equals the reference's own results on them
(tests/golden/mapbuild_sweep_pinned.npz, tests/tools/gen_mapbuild_sweep_pinned.py), and the probe-walk helper on the clash ids."""
import numpy as np
import pytest

from tests import mapbuild_ref as MR


def _filled(s):
    return [(len(p), t) for p, t in zip(s["landmarks"], s["traces"]) if len(p)]


def test_wide_reaches_every_shape_class():
    s = MR.sweep_scene("wide")
    rows = np.diff(s["frame_off"])
    assert s["F"] >= 600 and rows.min() == 0 and rows.max() <= 400 and ((rows > 0) & (rows < 64)).any() and (rows > 256).any()
    assert s["params"] == dict(min_obs=120, topk_imgs=260, n_vrf=10, min_cover_ratio=0.9, gain_floor=0.01)
    sizes = [len(p) for p in s["landmarks"]]
    assert [n for n in sizes if n] == list(MR.WIDE_SIZES)
    e = MR.WIDE_LM_EMPTY
    assert sizes[e] == 0 and sizes[e - 1] > 0 and sizes[e + 1] > 0 and s["vrf"][e] == []
    t = _filled(s)
    assert any(x["n_eligible"] > 260 and x["topk_cut"] and x["n_candidates"] == 260 and x["count_tie"] and x["gain_tie"] for _, x in t)
    assert {x["stop"] for _, x in t} == {"coverage", "gain floor", "n_vrf", "none left"}
    for key in ("ignored", "lacking", "repeated", "id0", "drop7", "drop8"):
        assert any(x.get(key) for _, x in t), key
    assert any(n > 256 and x["drop7"] for n, x in t) and any(n > 256 and x["drop8"] for n, x in t)
    assert max(x["n_encountered"] for _, x in t) > 256
    d = s["traces"][MR.WIDE_LM_DROPS]
    assert d["chosen"][:3] == [MR.WIDE_LACK_ONLY, MR.WIDE_AWAY, MR.WIDE_DEPTH0] and not set(d["chosen"][:3]) & set(s["vrf"][MR.WIDE_LM_DROPS])
    # the kernel's table names frames the map does not hold; the restatement's does not
    assert (s["pt_frames"] == -1).any() and (s["pt_frames"] == s["F"]).any()
    assert all(0 <= f < s["F"] for v in s["point_frames"].values() for f in v)
    assert (s["point3D_ids"] == 0).any() and (s["point3D_ids"] < -1).any()


def test_fallback_wide():
    s = MR.sweep_scene("fallback_wide")
    counts = [int((a > 0).sum()) for a in s["frame_point_ids"]]
    assert s["params"]["min_obs"] > max(counts) and s["params"]["topk_imgs"] == 3
    t = _filled(s)
    assert all(x["fallback"] and x["n_eligible"] == 0 and x["n_candidates"] == x["n_encountered"] for _, x in t)
    assert any(x["n_encountered"] > 256 for _, x in t)
    assert any(len(v) > len(set(v)) for v in s["point_frames"].values())      # a frame more than once in a point's list
    assert 0 in np.diff(s["frame_off"])


def test_n_vrf64():
    s = MR.sweep_scene("n_vrf64")
    assert s["params"] == dict(min_obs=120, topk_imgs=257, n_vrf=64, min_cover_ratio=1.0, gain_floor=0.0)
    t = _filled(s)
    assert all(x["repeated"] and x["stop"] != "coverage" for _, x in t)
    assert any(x["n_picks"] == 64 and x["stop"] == "n_vrf" for _, x in t)
    assert any(x["stop"] == "none left" and x["zero_gain"] and 1 < x["n_picks"] < 64 for _, x in t)
    assert any(x["n_eligible"] > 257 and x["n_candidates"] == 257 for _, x in t)
    assert any(len(v) == 64 for v in s["vrf"])


def test_big_ids_need_all_64_bits():
    s = MR.sweep_scene("big_ids")
    assert min(p for p in s["point_frames"]) >= 1 << 40 and all(i >= 1 << 40 for i in s["point3D_ids"].tolist() if i > 0)
    pairs = s["landmarks"][MR.BIG_LM_PAIRS]
    halves = [p for p in pairs if p + (1 << 32) in pairs]
    assert len(halves) == 5
    h = 2 * len(pairs) + 1
    for p in halves:      # both halves start their probe in the same slot, and sit on different frames
        assert MR.hash_id(p) % h == MR.hash_id(p + (1 << 32)) % h
        carried = lambda i: {f for f, a in enumerate(s["frame_point_ids"]) if i in a.tolist()}
        assert carried(p) and carried(p + (1 << 32)) and not carried(p) & carried(p + (1 << 32))
    vrf32, _ = MR.truncated_ids(s)
    assert vrf32[MR.BIG_LM_PAIRS] != s["vrf"][MR.BIG_LM_PAIRS] and s["vrf"][MR.BIG_LM_PAIRS] == [5, 4, 3]
    assert (s["point3D_ids"] < -1).any() and any(p < -1 for v in s["landmarks"] for p in v)


def test_clash_ids_share_a_slot_and_wrap():
    s = MR.sweep_scene("clash")
    ids = s["landmarks"][MR.CLASH_LM]
    h = 2 * len(ids) + 1
    assert len(ids) == MR.CLASH_N and h == 81 and len(set(ids)) == len(ids) and min(ids) > 0
    slot, start, steps = MR.probe_walk(ids)
    assert set(start.values()) == {MR.CLASH_SLOT}
    assert sorted(slot.values()) == sorted((MR.CLASH_SLOT + k) % h for k in range(len(ids)))      # one chain, over the table's end
    assert min(slot.values()) == 0 and max(slot.values()) == h - 1 and max(steps.values()) == len(ids) - 1
    seq = s["landmarks"][MR.CLASH_LM_SEQUENTIAL]
    assert seq == list(range(seq[0], seq[0] + len(seq)))
    assert len(set(MR.probe_walk(seq)[1].values())) > len(seq) // 2      # sequential ids spread out


def test_probe_walk_helper():
    assert MR.hash_id(1) == MR.HASH_MUL >> 32 and MR.hash_id(-1) == ((1 << 64) - MR.HASH_MUL) >> 32 and MR.hash_id(0) == 0
    a, b = MR.ids_starting_at(2, 5, 2)
    slot, start, steps = MR.probe_walk([a, b, a, 0, -3], h=5)
    assert slot == {a: 2, b: 3} and start == {a: 2, b: 2} and steps == {a: 0, b: 1}
    a, b, c = MR.ids_starting_at(4, 5, 3)
    assert MR.probe_walk([a, b, c], h=5)[0] == {a: 4, b: 0, c: 1}      # s + 1 == h -> 0


def test_degenerate_calls():
    c = MR.sweep_calls("degenerate")
    assert set(c) == {"all_empty", "F1", "cover0", "topk1", "n_vrf1"}
    assert c["all_empty"]["landmarks"] == [[], [], []] and c["F1"]["F"] == 1
    assert c["cover0"]["params"]["min_cover_ratio"] == 0.0 and all(v == [] and t.get("n_picks", 0) == 0 for v, t in zip(c["cover0"]["vrf"], c["cover0"]["traces"]))
    assert c["topk1"]["params"]["topk_imgs"] == 1 and all(t["n_candidates"] == 1 for _, t in _filled(c["topk1"]))
    assert c["n_vrf1"]["params"]["n_vrf"] == 1 and all(t["n_picks"] == 1 and t["stop"] == "n_vrf" for _, t in _filled(c["n_vrf1"]))
    assert any(v for v in c["F1"]["vrf"]) and any(v for v in c["topk1"]["vrf"])


@pytest.mark.parametrize("name", MR.SWEEP_NAMES)
def test_filter_verdicts_do_not_hang_on_rounding(name):
    """numpy's 4 x 4 product and the kernel's written-out sum may differ in the last bit: no verdict may depend on it."""
    seen = 0
    for tag, s in MR.sweep_calls(name).items():
        v = MR.filter_verdicts(s)
        assert all(x[3] for x in v), (tag, [x for x in v if not x[3]])
        seen += len(v)
    assert seen > 0 or name == "degenerate"
    if name == "wide":
        v = MR.filter_verdicts(MR.sweep_scene("wide"))
        assert (MR.WIDE_LM_DROPS, MR.WIDE_AWAY, False, True) in v and (MR.WIDE_LM_DROPS, MR.WIDE_DEPTH0, False, True) in v


@pytest.mark.parametrize("name", MR.SWEEP_PINNED)
def test_restatement_reproduces_the_reference_on_the_sweep(golden, name):
    g, s = golden("mapbuild_sweep_pinned"), MR.sweep_scene(name)
    assert int(g["seed"]) == MR.SEED and s["params"]["gain_floor"] == 0.01
    vrf, n = g[name + "_vrf"], g[name + "_vrf_n"]
    assert vrf.shape == (len(s["landmarks"]), s["params"]["n_vrf"])
    for l, want in enumerate(s["vrf"]):
        assert vrf[l, :n[l]].tolist() == want and (vrf[l, n[l]:] == -1).all(), (name, l)


def test_long_track_scene_reaches_every_storage_regime():
    s = MR.long_track_scene()
    assert MR.IDX_LDS == MR.SHORT * 128 == 4096
    length = lambda name: int(s["trk_off"][s["special"][name] + 1] - s["trk_off"][s["special"][name]])
    kept = lambda name: s["medians"][s["special"][name]][0]
    for n in (4095, 4096, 4097, 5000):
        name = f"len{n}"
        assert length(name) == n and len(kept(name)) <= 48 and kept(name)[0] == 0 and kept(name)[-1] == n - 1
        assert s["trk_off"][s["special"][name]] != 0
        if n > 4096:
            assert 4095 in kept(name) and 4096 in kept(name)
    assert len(kept("len4095")) % 2 == 1 and len(kept("len4096")) % 2 == 0
    for n in (600, 513, 512):
        name = f"len{n}_dropped"
        assert length(name) == n and 0.3 < 1 - len(kept(name)) / n < 0.36
    i = s["special"]["repeat_long"]
    pos, med = s["medians"][i]
    rows = MR.entry_rows(s["frame_off"].astype(np.int64), s["trk_frame"], s["trk_kpt"])[s["trk_off"][i]:s["trk_off"][i + 1]][pos]
    assert length("repeat_long") > MR.ROW_LDS and len(set(rows.tolist())) == len(rows) - 1 and med[9] == med[41]
    # short tracks on both sides of the long ones: the workspace ends before the entries do, and with them when cut at n_prefix
    lens = np.diff(s["trk_off"])
    P = s["n_prefix"]
    assert lens[0] <= MR.SHORT and lens[-1] <= MR.SHORT and lens[P - 1] > MR.SHORT and (lens[P:] <= MR.SHORT).all()
    assert (s["choice"][[s["special"][k] for k in s["special"]]] >= 0).all()
