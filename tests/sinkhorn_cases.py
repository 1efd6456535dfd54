"""Inputs of the Sinkhorn / dual-softmax sweep, shared by tests/test_sinkhorn_inputs_cpu.py (which proves that every one of
them is well conditioned: the fp32 oracle stays inside the plan bars against fp64) and tests/test_gpu_sinkhorn_sweep.py
(which holds the device to the same bars).  Nothing here touches a device.

Shape classes follow the structure of pram_amd/csrc/sinkhorn.hip:
  - four kernel instantiations chosen by ldw = roundup4(n + 1): NV = 2, 5, 9, 17 for ldw <= 512, 1280, 2304, 4352;
  - 32 row blocks of ceil((m + 1) / 32) rows, four waves each, one row's result kept per lane (m <= 8191).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import torch

from oracle import ref_cpu as R
from pram_amd import weights as W

BINS = (-3.0, 0.0, 1.0, 4.5)
THRESHOLDS = (0.0, 0.2)
SINK_ABS, SINK_REL = 1e-6, 2e-6      # |p - ref| - SINK_REL * |ref| < SINK_ABS   (the bar of test_sinkhorn_golden / _2049)
DUAL_ABS = 1e-5                      # |p - ref| < DUAL_ABS                       (the bar of test_sinkhorn_golden)
M_LIMIT, N_LIMIT = 8191, 4351


def nv_of(n: int) -> int:
    """The instantiation that serves n columns."""
    ldw = (n + 1 + 3) // 4 * 4
    for nv in (2, 5, 9, 17):
        if ldw <= nv * 256:
            return nv
    raise ValueError(n)


@dataclass(frozen=True)
class Case:
    kind: str                 # "col" | "row" | "mid" | "iter"
    m: int
    n: int
    bin: float
    iters: int = 20
    ties: Tuple[Tuple[int, int, int, int], ...] = ()      # (rA, rB, cA, cB): rows rA == rB, columns cA == cB, all four entries the maximum

    @property
    def id(self) -> str:
        return f"{self.kind}-{self.m}x{self.n}-it{self.iters}-bin{self.bin:g}" + ("-ties" if self.ties else "")

    @property
    def nv(self) -> int:
        return nv_of(self.n)


def _block_ties(m: int, n: int):
    """Two planted 2 x 2 ties for a problem whose row blocks hold at least five rows.  The first pair of rows sits in ONE row
    block with the lower row in the later wave (rows rbeg + 1 and rbeg + 4: column partial 4 * blk + 1 and 4 * blk + 0), so
    the column arg-max meets the higher row first and only the lowest-index rule picks the right one; the second pair spans
    the first and the last block.  The columns of each pair sit in different lanes, the last one on the dust-bin edge."""
    rpb = (m + 1 + 31) // 32
    assert rpb >= 5
    rbeg = 3 * rpb
    return ((rbeg + 1, rbeg + 4, 3, n // 2), (2, m - 1, 1, n - 1))


def _cases():
    out = []
    ms = (5, 9, 17, 26, 33, 40)
    edge_ties = {4, 512, 1280, 2304, 4351}
    for k, n in enumerate((1, 2, 3, 4, 63, 64, 255, 256, 507, 508, 511, 512, 1279, 1280, 2303, 2304, 4351)):
        m = ms[k % len(ms)]
        out.append(Case("col", m, n, BINS[k % 4], ties=((0, m - 1, 0, n - 1),) if n in edge_ties else ()))
    k = 0
    for m in (1, 30, 31, 32, 33, 127, 128, 129, 4351, 8191):
        for n in (8, 70):
            k += 1
            out.append(Case("row", m, n, BINS[k % 4], ties=((1, m - 2, 0, n - 1),) if m in (33, 129) else ()))
    mids = ((300, 511), (300, 1000), (600, 2303), (300, 4351))
    for k, (m, n) in enumerate(mids):
        out.append(Case("mid", m, n, BINS[(k + 1) % 4], ties=_block_ties(m, n)))
    for k, (m, n) in enumerate(mids):
        for it in (0, 1, 100):
            out.append(Case("iter", m, n, BINS[(k + it) % 4], iters=it))
    return tuple(out)


CASES = _cases()
BATCH = 2


def sink_input(tag: str, batch: int, m: int, n: int, ties=()) -> torch.Tensor:
    """N(0, 2^2) scores with a planted partial permutation of +6 (the idiom of _sink_input in test_gpu_kernels.py), then the
    planted exact ties: a value of 16 at (rA, cA) (above anything noise plus plant reaches), column cA copied to cB and row
    rA copied to rB."""
    M = W.normal(31, f"sweep/{tag}", (batch, m, n), 2.0)
    k = min(m, n)
    for b in range(batch):
        idx = torch.argsort(W.uniform(32 + b, f"sweep/perm/{tag}", (m,)))[:k]
        M[b, idx, torch.arange(k)] += 6.0
    for rA, rB, cA, cB in ties:
        M[:, rA, cA] = 16.0
    for rA, rB, cA, cB in ties:
        M[:, :, cB] = M[:, :, cA]
    for rA, rB, cA, cB in ties:
        M[:, rB, :] = M[:, rA, :]
    return M


def case_input(c: Case) -> torch.Tensor:
    return sink_input(f"{c.kind}/{c.m}x{c.n}", BATCH, c.m, c.n, c.ties)


def reference(M: torch.Tensor, bin_score: float, iters: int, dual: bool, dtype=torch.float64) -> torch.Tensor:
    """The oracle in ``dtype`` (it follows the dtype of its input)."""
    x, bs = M.to(dtype), torch.tensor(bin_score, dtype=dtype)
    return R.dual_softmax(x, bs) if dual else R.sink_algorithm(x, bs, iters)


def deviation(p: torch.Tensor, ref: torch.Tensor, dual: bool) -> float:
    """The figure each bar is about: max |p - ref| (dual, bar DUAL_ABS) or max (|p - ref| - SINK_REL |ref|) (Sinkhorn, bar
    SINK_ABS; negative when every entry is inside the relative part alone)."""
    d = (p.double() - ref.double()).abs()
    if not dual:
        d = d - SINK_REL * ref.double().abs()
    return float(d.max())


def abs_rel(p: torch.Tensor, ref: torch.Tensor):
    """(max |p - ref|, max |p - ref| / |ref|): reported beside the bar's own figure, never asserted."""
    d = (p.double() - ref.double()).abs()
    return float(d.max()), float((d / ref.double().abs().clamp_min(1e-300)).max())


def bar(dual: bool) -> float:
    return DUAL_ABS if dual else SINK_ABS


# ---- ragged batches ------------------------------------------------------------------------------------------------
# (m_max, n_max): n_max in the NV = 5 and NV = 9 instantiations, neither a multiple of 4 (the n_valid < ldd case pads them)
RAGGED_SHAPES = ((70, 603), (45, 1301))


def ragged_lens(m_max: int, n_max: int):
    """Full size, an empty side each way, 1 x 1, a single column under every row, and an interior pair."""
    return ((m_max, n_max), (0, n_max), (m_max, 0), (1, 1), (m_max, 1), (m_max // 2 + 2, n_max // 2 + 31))


def ragged_input(m_max: int, n_max: int) -> torch.Tensor:
    return sink_input(f"ragged/{m_max}x{n_max}", 6, m_max, n_max)


RAGGED_BIN = {603: 4.5, 1301: -3.0}

# ---- grouping: B = 9 ragged pairs that run as groups of 4, 4 and 1 -------------------------------------------------
GROUP_SHAPE = (50, 90)
GROUP_LENS = ((50, 90), (41, 88), (50, 77), (33, 35), (17, 61), (50, 9), (29, 64), (3, 5), (44, 81))


def group_input() -> torch.Tensor:
    return sink_input("group", 9, *GROUP_SHAPE)
