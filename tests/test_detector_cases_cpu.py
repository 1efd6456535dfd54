"""CPU: the cases of the detector sweep (tests/detector_cases.py) reach what they name.  A sweep case that quietly misses its
branch hides a failure, so everything tests/test_gpu_detector_sweep.py relies on is asserted here from the reference alone
(oracle/ref_cpu.py and numpy): candidate counts against k, the fallback decision, the exact thresholds, the shape of the tie
groups, the global-memory sort's range, that the suppression rounds of simple_nms matter on the lattices, that the seam cases
keep pixels on both sides of a tile seam, and that the fp32 oracle of the score map sits inside the derived bar."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import detector_cases as D

SEL = D.sel_cases() + [D.sel_regime_batch()]


# ------------------------------------------------------------------------------------------------ score map
def test_score_shapes_cover_every_remainder_of_the_cell_guard():
    assert sorted({b * h * w % 4 for b, h, w in D.SCORE_SHAPES}) == [0, 1, 2, 3]
    assert any(h > w for _, h, w in D.SCORE_SHAPES) and any(h < w for _, h, w in D.SCORE_SHAPES)


def test_score_reference_is_the_float64_softmax_in_depth_to_space_order():
    """the module's own depth-to-space (used for the bar) agrees with the oracle's, so bar and reference line up element by
    element; the one-hot case puts its peak where the formula says"""
    lg = D.score_logits((2, 3, 3), "normal")
    assert torch.equal(D._depth_to_space(torch.softmax(lg.double(), 1)[:, :64]), D.score_reference(lg))
    hot = D.score_logits((2, 12, 16), "one_hot")
    ch = hot.argmax(1)      # channel of the maximum of every cell
    assert set(ch.unique().tolist()) >= {0, 63} and int(ch.max()) < 64
    ref = D.score_reference(hot)
    cy, cx, c = 5, 7, int(ch[1, 5, 7])
    assert float(ref[1, 8 * cy + c // 8, 8 * cx + c % 8]) > 0.99


@pytest.mark.parametrize("regime", list(D.SCORE_REGIMES))
def test_score_oracle_inside_the_bar(regime):
    """torch's fp32 softmax against float64 under (|x - mx| + SCORE_CONST) * 2^-24: the bar is derived, and the fp32 oracle —
    which is not the code under test — must fit it on every case, or the bar asks for more than fp32 can give."""
    worst, reach, share = 0.0, 0.0, 0.0
    for shape in D.SCORE_SHAPES:
        lg = D.score_logits(shape, regime)
        ratio, tiny = D.score_ratio(R.score_map_from_logits(lg), lg)
        worst, share = max(worst, ratio), max(share, tiny)
        live = D.score_reference(lg) >= D.SCORE_TINY
        reach = max(reach, float((D.score_bar(lg)[live] * 2.0 ** 24 - D.SCORE_CONST).max()))
        err = ((R.score_map_from_logits(lg).double() - D.score_reference(lg)).abs() / D.score_reference(lg))[live].max().item()
        print(f"score map oracle {regime} {shape}: error / bar = {ratio:.3f}, largest relative error {err * 2 ** 24:.1f} x 2^-24, "
              f"largest |x - mx| above the cut {reach:.1f}, share below the cut = {tiny:.3f}")
    assert worst <= 1.0, (regime, worst)
    if regime == "wide":
        assert 0.0 < share <= 0.60, share          # the regime underflows somewhere, and most of it is still compared
        assert reach > 60.0                         # and the compared part reaches down to where only mx keeps expf finite
    if regime == "normal":
        assert share == 0.0
    if regime == "dustbin":
        lg = D.score_logits((2, 12, 16), regime)
        assert bool((lg.argmax(1) == 64).all()) and float(D.score_reference(lg).max()) < 1e-6
    if regime == "equal":
        assert torch.equal(D.score_reference(D.score_logits((1, 3, 5), regime)), torch.full((1, 24, 40), 1.0 / 65.0, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ simple_nms
def test_nms_table_covers_what_the_issue_lists():
    cases = D.nms_cases()
    assert len({c[0] for c in cases}) == len(cases)
    for shape in ((2, 31, 33), (3, 45, 77)):
        assert {c[2] for c in cases if c[1] == shape} == set(D.NMS_CONTENTS)
    assert {c[1] for c in cases if c[2] == "plateau"} == set(D.NMS_SHAPES)
    sides = {s for _, h, w in D.NMS_SHAPES for s in (h, w)}
    assert {1, 31, 32, 33} <= sides and any(s > 2 * D.NMS_TILE for s in sides)


@pytest.mark.parametrize("radius", [r for r in D.NMS_RADII if r > 0])
def test_nms_lattice_needs_the_suppression_rounds(radius):
    """on the dense lattice the first mask alone loses peaks that the two rounds bring back; on the far lattice (r + 1 apart)
    every peak is alone in its window and survives — one pixel closer and it would not"""
    n = 0
    for name, shape, content in D.nms_cases():
        if content == "lattice":
            s = D.nms_map(shape, content, radius)
            full, first = R.simple_nms(s, radius), D.first_mask_only(s, radius)
            assert not torch.equal(full, first), name
            assert int((full > 0).sum()) > int((first > 0).sum()) and int((full > 0).sum()) < int((s > 0).sum()), name
            n += 1
        elif content == "lattice_far":
            s = D.nms_map(shape, content, radius)
            assert torch.equal(R.simple_nms(s, radius), s) and int((s > 0).sum()) > 4, name
            n += 1
    assert n == 4


@pytest.mark.parametrize("radius", D.NMS_RADII)
def test_nms_seam_cases_keep_pixels_on_both_sides_of_a_seam(radius):
    seam = D.nms_seam_cases()
    assert len(seam) == 3
    for name, shape, content in seam:
        kept = R.simple_nms(D.nms_map(shape, content, radius), radius) > 0
        for line in (31, 32):
            assert bool(kept[:, line, :].any()) and bool(kept[:, :, line].any()), (name, line)
        assert bool(kept[:, 31, 40].all()) and bool(kept[:, 32, 40].all()), name          # the equal pair across the row seam
        assert bool(kept[:, 0, 0].all()) and bool(kept[:, -1, -1].all()) and bool(kept[:, 0, -1].all()) and bool(kept[:, -1, 0].all()), name
        if shape[1] > 40:
            assert bool(kept[:, 40, 31].all()) and bool(kept[:, 40, 32].all()), name      # and across the column seam


def test_nms_plateau_and_constant_maps_tie():
    s = D.nms_map((3, 45, 77), "plateau", 2)
    assert len(s.unique()) == 8
    assert torch.equal(R.simple_nms(D.nms_map((2, 31, 33), "constant", 4), 4), D.nms_map((2, 31, 33), "constant", 4))


# ------------------------------------------------------------------------------------------------ selection
def test_selection_table_covers_what_the_issue_lists():
    assert len({c.name for c in SEL}) == len(SEL)
    assert {tuple(c.nms.shape[1:]) for c in SEL} == set(D.SEL_MAPS)
    assert {c.nms.shape[0] for c in SEL} == {1, 2, 3}
    assert max(c.nms.numel() for c in SEL) == 2 * 120 * 160
    assert {(8, 4), (9, 4), (40, 20), (61, 30)} <= {(c.nms.shape[1], c.border) for c in SEL}      # border = h // 2
    assert {0, 4} <= {c.border for c in SEL}
    big = {c.k for c in SEL if c.count == ">"}
    assert {1, 1024, 1025, 8192, 8193, 10000} <= big
    assert any(c.k >= c.nms.shape[1] * c.nms.shape[2] for c in SEL)
    assert {c.fallback_ref for c in SEL} >= {-1, 0, 1, 2}
    assert any(c.nms.shape[1] * c.nms.shape[2] < D.SEL_SLABS * 8 for c in SEL)
    assert any(c.nms.shape[1] * c.nms.shape[2] % 8 for c in SEL) and any(c.nms.shape[2] % 8 for c in SEL)
    assert all(bool((c.nms >= 0).all()) and c.nms.dtype == torch.float32 and c.nms.is_contiguous() for c in SEL)


@pytest.mark.parametrize("case", SEL, ids=lambda c: c.name)
def test_selection_case_reaches_its_branch(case):
    kps, scs = D.sel_reference(case)
    stats = D.sel_stats(case)
    B, h, w = case.nms.shape
    for b in range(B):
        st, c = stats[b], len(scs[b])
        # the numpy restatement of the candidate list is the reference's: same count, and the same scores when nothing is cut
        assert c == min(len(st["cand"]), case.k) and len(kps[b]) == c, (b, c)
        if len(st["cand"]) <= case.k:
            assert np.array_equal(st["cand"], scs[b].numpy())
        n = len(st["cand"])
        if case.count is not None:
            assert {"<": n < case.k, "==": n == case.k, "==k+1": n == case.k + 1, ">": n > case.k}[case.count], (b, n, case.k)
        if case.low is not None:
            assert st["low"] == case.low[b], (b, st["cnt_hi"], case.min_kp)
        if "candidates" in case.claims:
            assert n == case.claims["candidates"], (b, n)
        if "cnt_hi" in case.claims:
            assert st["cnt_hi"] == case.claims["cnt_hi"][b]
        if "kept" in case.claims:
            assert scs[b].tolist() == [float(np.float32(v)) for v in case.claims["kept"]]
        if case.claims.get("row_cross"):
            first = case.border * w                       # first pixel of the first interior row: not at the start of a run of 8 ...
            run_end = first // 8 * 8 + 8
            assert first % 8 and run_end - first > case.border                            # ... and the run reaches interior columns
            inner = [x for x in range(case.border, run_end - first) if x < w - case.border]
            assert inner and all(any((kps[b] == torch.tensor([float(x), float(case.border)])).all(1)) for x in inner)
        if case.claims.get("global_sort"):
            assert D.SEL_LDS_K < case.k < h * w and n > case.k
        if case.claims.get("straddle"):
            n_gt, n_eq, take, pos = D.tie_split(st["cand"], case.k)
            assert 0 < take < n_eq and n_gt > 0
            taken, left = set((pos[:take] // D.SEL_WG).tolist()), set((pos[take:] // D.SEL_WG).tolist())
            assert len(taken) >= 2 and len(left) >= 2, (taken, left)
            assert len(set((pos // D.SEL_WG).tolist())) == -(-n // D.SEL_WG)           # the group has members in every chunk
            assert pos[take - 1] // D.SEL_WG == pos[take] // D.SEL_WG                   # the cut falls inside a chunk
            print(f"{case.name}: {n} candidates, {n_gt} above the k-th score, {n_eq} equal to it over chunks "
                  f"{sorted(set((pos // D.SEL_WG).tolist()))}, {take} taken, cut in chunk {pos[take] // D.SEL_WG}")
        if case.claims.get("all_equal"):
            assert len(np.unique(st["cand"])) == 1 and n > case.k
            assert torch.equal(kps[b][:, 1] * w + kps[b][:, 0], torch.sort(kps[b][:, 1] * w + kps[b][:, 0]).values)
        if case.claims.get("low_byte"):
            bits = np.unique(st["cand"].view(np.uint32))
            assert len(bits) > 200 and len(np.unique(bits >> 8)) == 1
            n_gt, n_eq, take, _ = D.tie_split(st["cand"], case.k)
            assert 0 < take <= n_eq and n_gt > 0


def test_selection_fallback_cases_sit_on_the_edge_of_the_test():
    by = {c.name: c for c in SEL}
    at, plus = D.sel_stats(by["fallback-at-min"]), D.sel_stats(by["fallback-at-min+1"])
    assert at[0]["cnt_hi"] == by["fallback-at-min"].min_kp and plus[0]["cnt_hi"] == by["fallback-at-min+1"].min_kp + 1
    assert len(at[0]["cand"]) > len(plus[0]["cand"]) > 0
    # the fallback count ignores the border: fewer of the high pixels are candidates than were counted
    assert len(plus[0]["cand"]) == plus[0]["cnt_hi"] - 4
    per = D.sel_stats(by["fallback-per-frame"])
    assert {s["low"] for s in per} == {True, False}
    assert per[2]["cnt_hi"] == by["fallback-per-frame"].min_kp          # a frame of the batch exactly at the edge
    # under fallback_ref = j every frame follows frame j, against its own count
    for name, ref in (("fallback-ref-1", 1), ("fallback-ref-2", 2)):
        st = D.sel_stats(by[name])
        assert all(s["low"] for s in st) and st[0]["cnt_hi"] > by[name].min_kp >= st[ref]["cnt_hi"]
    assert any(len(s["cand"]) > by["fallback-ref-2"].k for s in D.sel_stats(by["fallback-ref-2"]))


def test_selection_reference_compares_thresholds_in_fp32():
    """np.float32(conf_th) and np.float32(conf_th) * 0.5 pass the reference's >=, their predecessors do not"""
    th = np.float32(D.CONF_TH)
    v = torch.from_numpy(np.array([th, D._prev(th), th * np.float32(0.5), D._prev(th * np.float32(0.5))], dtype=np.float32))
    assert (v >= D.CONF_TH).tolist() == [True, False, False, False]
    assert (v >= D.CONF_TH * 0.5).tolist() == [True, True, True, False]
    assert float(th) != D.CONF_TH and float(th * np.float32(0.5)) == float(th) * 0.5


def test_selection_regime_batch_has_the_three_regimes():
    c = D.sel_regime_batch()
    n = [len(s["cand"]) for s in D.sel_stats(c)]
    assert 0 < n[0] <= c.k < n[1] and n[2] == 0
