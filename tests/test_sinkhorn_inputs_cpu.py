"""CPU: the conditions on the inputs of the Sinkhorn / dual-softmax sweep (tests/test_gpu_sinkhorn_sweep.py), and the two
argument limits of the C entry, which are refused before anything touches a device.

The sweep holds the device's plan to the bars the suite already uses against the fp32 goldens.  Those bars are fair only for
inputs on which fp32 arithmetic itself can meet them, so this file asserts, for the exact inputs of the sweep, that the fp32
oracle stays inside both bars against the fp64 oracle: an ill-conditioned input is rejected here, not excused on the GPU."""
import ctypes

import pytest
import torch

from tests import sinkhorn_cases as S


def _classes():
    seen = {}
    for c in S.CASES:
        seen.setdefault((c.kind, c.nv), []).append(c)
    return seen


CLASSES = _classes()


def test_case_list_reaches_every_structure():
    """The sweep's shape list covers what the issue names: every instantiation edge, the row-block classes, all four bin
    scores, every iteration count at every instantiation, and planted ties at every instantiation."""
    cols = {c.n for c in S.CASES if c.kind == "col"}
    assert cols == {1, 2, 3, 4, 63, 64, 255, 256, 507, 508, 511, 512, 1279, 1280, 2303, 2304, 4351}
    assert all(5 <= c.m <= 40 for c in S.CASES if c.kind == "col")
    rows = {(c.m, c.n) for c in S.CASES if c.kind == "row"}
    assert rows == {(m, n) for m in (1, 30, 31, 32, 33, 127, 128, 129, 4351, 8191) for n in (8, 70)}
    assert {c.bin for c in S.CASES} == set(S.BINS)
    assert [S.nv_of(n) for n in (511, 512, 1279, 1280, 2303, 2304, 4351)] == [2, 5, 5, 9, 9, 17, 17]
    for nv in (2, 5, 9, 17):
        assert {c.iters for c in S.CASES if c.nv == nv and c.kind in ("mid", "iter")} == {0, 1, 20, 100}
        assert any(c.ties for c in S.CASES if c.nv == nv and c.kind == "mid")
        assert any(c.ties for c in S.CASES if c.nv == nv and c.kind == "col")
    assert max(c.m for c in S.CASES) == S.M_LIMIT and max(c.n for c in S.CASES) == S.N_LIMIT
    assert len({c.id for c in S.CASES}) == len(S.CASES)
    for c in S.CASES:
        if c.kind == "mid":      # rows up to the last or last-but-one block, and a tie pair inside one block with the lower row in the later wave
            rpb = (c.m + 1 + 31) // 32
            assert (c.m + 1 + rpb - 1) // rpb >= 31
            rA, rB = c.ties[0][:2]
            assert rA // rpb == rB // rpb and rA < rB and (rA % rpb) % 4 > (rB % rpb) % 4


@pytest.mark.parametrize("key", sorted(CLASSES), ids=lambda k: f"{k[0]}-NV{k[1]}")
def test_fp32_oracle_meets_the_plan_bars(key):
    """fp32 oracle against fp64 oracle, both paths, on every input of the class: inside the bars the device is held to.  The
    planted ties are ties of the plan too: the four entries agree and strictly dominate their rows and columns."""
    worst = {False: -1.0, True: -1.0}
    for c in CLASSES[key]:
        M = S.case_input(c)
        for dual in (False, True):
            if dual and c.iters != 20:
                continue      # the dual path has no iterations: one run per shape
            ref = S.reference(M, c.bin, c.iters, dual)
            d = S.deviation(S.reference(M, c.bin, c.iters, dual, torch.float32), ref, dual)
            worst[dual] = max(worst[dual], d)
            assert d < S.bar(dual), (c.id, dual, d)
            for rA, rB, cA, cB in c.ties:
                inner = ref[:, :-1, :-1]
                blk = inner[:, [rA, rA, rB, rB], [cA, cB, cA, cB]]
                assert float((blk.max(1).values / blk.min(1).values).max()) < 1 + 1e-9, c.id
                rest = inner.clone()
                rest[:, [rA, rB], cA] = 0
                rest[:, [rA, rB], cB] = 0
                for r_ in (rA, rB):
                    assert bool((rest[:, r_, :].max(1).values < blk.min(1).values * (1 - 1e-4)).all()), (c.id, "row", r_)
                rest = inner.clone()
                rest[:, rA, [cA, cB]] = 0
                rest[:, rB, [cA, cB]] = 0
                for c_ in (cA, cB):
                    assert bool((rest[:, :, c_].max(1).values < blk.min(1).values * (1 - 1e-4)).all()), (c.id, "col", c_)
    print(f"{key}: fp32 oracle vs fp64, sinkhorn excess {worst[False]:.3e}, dual |d| {worst[True]:.3e}")


@pytest.mark.parametrize("m_max,n_max", S.RAGGED_SHAPES)
def test_fp32_oracle_meets_the_plan_bars_ragged(m_max, n_max):
    M = S.ragged_input(m_max, n_max)
    for b, (m, n) in enumerate(S.ragged_lens(m_max, n_max)):
        for dual in (False, True):
            sub = M[b:b + 1, :m, :n]
            d = S.deviation(S.reference(sub, S.RAGGED_BIN[n_max], 20, dual, torch.float32),
                            S.reference(sub, S.RAGGED_BIN[n_max], 20, dual), dual)
            assert d < S.bar(dual), (m, n, dual, d)


def test_grouping_lengths_differ_between_groups():
    """Groups of four: a call that forgot to slice the lengths would hand pairs 4..7 the lengths of pairs 0..3."""
    L = S.GROUP_LENS
    assert len(L) == 9 and all(L[b] != L[b - 4] for b in range(4, 9))
    assert all(L[b][0] != L[b - 4][0] and L[b][1] != L[b - 4][1] for b in range(4, 8))
    assert all(1 <= m <= S.GROUP_SHAPE[0] and 1 <= n <= S.GROUP_SHAPE[1] for m, n in L)


# ---- argument limits: refused before the batch == 0 return, so no device is needed -----------------------------------
def _entry_rc(lib, dual, m_max, n_max, ldp=None, with_p=False):
    buf = ctypes.create_string_buffer(64)      # non-null stand-ins: with batch == 0 nothing is dereferenced or launched
    ptr = ctypes.addressof(buf)
    p_out, ldp = (ptr if with_p else None), (n_max + 1 if ldp is None else ldp)
    if dual:
        return lib.pram_dual_softmax_match_f32(ptr, n_max, None, None, ptr, 0.2, p_out, ldp, None, None, None, None, 0, m_max, n_max, ptr, None)
    return lib.pram_sinkhorn_match_f32(ptr, n_max, None, None, ptr, 20, 0.2, p_out, ldp, None, None, None, None, 0, m_max, n_max, ptr, None)


@pytest.mark.parametrize("dual", [False, True], ids=["sinkhorn", "dual"])
def test_size_limits_are_refused_without_a_device(hip_lib, dual):
    assert _entry_rc(hip_lib, dual, S.M_LIMIT, S.N_LIMIT, with_p=True) == 0
    assert _entry_rc(hip_lib, dual, S.M_LIMIT + 1, 8) == -1                      # PRAM_E_ARG
    assert b"8191 rows" in hip_lib.pram_last_error()
    assert _entry_rc(hip_lib, dual, 8, S.N_LIMIT + 1) == -1
    assert b"4351 columns" in hip_lib.pram_last_error()
    assert _entry_rc(hip_lib, dual, 8, 8, ldp=8, with_p=True) == -1              # ldp < n_max + 1
    assert b"ldp" in hip_lib.pram_last_error()
    assert _entry_rc(hip_lib, dual, 8, 8, ldp=9, with_p=True) == 0
