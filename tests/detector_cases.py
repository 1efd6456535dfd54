"""Inputs of the detector post-processing sweep (score map, simple_nms, keypoint selection: pram_amd/csrc/sfd2_post.hip), shared
by tests/test_detector_cases_cpu.py (which proves from the reference alone that every case reaches the branch it names) and
tests/test_gpu_detector_sweep.py (which holds the kernels to the reference on them).  Nothing here touches a device; the inputs
are seeded with pram_amd.weights, as tests/glue_ref.py seeds its cases.

Every case carries a name and the branch of the kernel it is there to reach.  The constants the branches turn on:
  score map   one wave per 8 x 8 cell, four cells per workgroup (guard: cell >= ncell);
  simple_nms  32 x 32 output tiles with a halo of the radius, radius 0 .. 4;
  selection   64 pixel slabs per frame (count / compaction, 8 pixels per thread), one workgroup of 1024 threads per frame for
              the radix select and the sort, sorted in LDS up to a bound of 8192 and in global memory beyond."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import ref_cpu as R
from pram_amd import weights as W

# ================================================================================================ score map
SCORE_SHAPES = ((1, 1, 1), (2, 3, 3), (1, 3, 5), (2, 12, 16), (1, 5, 2))      # (B, hc, wc): B * hc * wc mod 4 = 1, 2, 3, 0, 2
SCORE_REGIMES = {
    "normal": "logits of sigma 3: the everyday range of the detector head",
    "wide": "logits of sigma 40: only the subtraction of the cell's maximum keeps expf finite",
    "dustbin": "channel 64 at +30: the dustbin (lane 0's second value) carries the cell's maximum and nearly all of its sum",
    "one_hot": "one of the 64 pixel channels at +30, a different one in every cell (lanes 0 and 63 among them)",
    "equal": "all 65 logits of a cell equal: every score is 1 / 65",
}
SCORE_CONST = 16.0            # the bar's constant, in units of 2^-24 (see score_bar)
SCORE_TINY = 2.0 ** -126      # fp32's smallest normal number: float64 scores below it are only required to come out below 2 * SCORE_TINY


def score_logits(shape: Tuple[int, int, int], regime: str) -> torch.Tensor:
    """fp32 logits [B, 65, hc, wc] (the reference's layout; the kernel takes them NHWC)."""
    B, hc, wc = shape
    seed, full = 9100 + 100 * B + 10 * hc + wc, (B, 65, hc, wc)
    if regime == "wide":
        return W.normal(seed, "sm/wide", full, 40.0)
    if regime == "equal":
        return (W.uniform(seed, "sm/eq", (B, 1, hc, wc)) * 10.0).expand(full).contiguous()
    x = W.normal(seed, "sm/" + regime, full, 3.0)
    if regime == "dustbin":
        x[:, 64] += 30.0
    elif regime == "one_hot":
        cell = torch.arange(B * hc * wc).reshape(B, 1, hc, wc)
        x.scatter_add_(1, (cell * 7 + 63) % 64, torch.full((B, 1, hc, wc), 30.0))      # cell 0: channel 63, cell 55: channel 0
    elif regime != "normal":
        raise ValueError(regime)
    return x


def _depth_to_space(semi: torch.Tensor) -> torch.Tensor:
    """[B, 64, hc, wc] -> [B, 8 hc, 8 wc]: out[b, 8 cy + i, 8 cx + j] = semi[b, 8 i + j, cy, cx] (nets/sfd2.py:297-300)."""
    B, _, hc, wc = semi.shape
    out = torch.empty(B, hc * 8, wc * 8, dtype=semi.dtype)
    for i in range(8):
        for j in range(8):
            out[:, i::8, j::8] = semi[:, 8 * i + j]
    return out


def score_reference(logits: torch.Tensor) -> torch.Tensor:
    """float64 softmax over the 65 channels of the same fp32 logits, then depth-to-space."""
    return R.score_map_from_logits(logits.double())


def score_bar(logits: torch.Tensor) -> torch.Tensor:
    """Bar on the RELATIVE error of every score, derived and not measured: (|x - mx| + SCORE_CONST) * 2^-24 for an element with
    logit x in a cell whose maximum (dustbin included) is mx.  |x - mx| * 2^-24 is the rounding of the fp32 argument x - mx
    carried through exp; the constant covers expf (at most 2 ulp), the seven-level wave sum of the 64 exponentials, the second
    expf of the dustbin and one correctly rounded division: about 12 units of 2^-24."""
    x = logits.double()
    return (_depth_to_space((x.max(1, keepdim=True).values - x)[:, :64]) + SCORE_CONST) * 2.0 ** -24


def score_ratio(got: torch.Tensor, logits: torch.Tensor) -> Tuple[float, float]:
    """-> (largest |got - ref| / (bar * ref) over the elements whose float64 score is at least SCORE_TINY, share of the elements
    below it).  Every element is looked at; the ones below SCORE_TINY must come out in [0, 2 * SCORE_TINY)."""
    ref, bar = score_reference(logits), score_bar(logits)
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "a score that is not finite"
    tiny = ref < SCORE_TINY
    assert bool(((got[tiny] >= 0) & (got[tiny] < 2 * SCORE_TINY)).all()), "a score below the smallest normal number came out at or above twice it"
    big = ~tiny
    ratio = ((got[big] - ref[big]).abs() / (bar[big] * ref[big])).max().item() if bool(big.any()) else 0.0
    return ratio, tiny.double().mean().item()


# ================================================================================================ simple_nms
NMS_RADII = (0, 1, 2, 3, 4)
NMS_TILE = 32
NMS_SHAPES = ((1, 1, 1), (1, 1, 70), (1, 70, 1), (2, 31, 33), (1, 32, 32), (1, 33, 64), (3, 45, 77), (1, 65, 97))
NMS_CONTENTS = {
    "random": "continuous scores: a unique maximum in every window",
    "plateau": "floor(8 u) / 8: exact ties everywhere, the == of every stage decides",
    "constant": "one value: every pixel is a maximum of its window, nothing is ever suppressed",
    "zeros": "all zeros: the suppressed-score pool ties with the zeros it wrote",
    "peaks": "single peaks in the four corners and in rows and columns 31 and 32, equal pairs across both seams, low noise below",
    "lattice": "peaks r // 2 + 1 apart, decreasing in row-major order: each sits in the window of a higher one, so only the "
               "suppression rounds bring back the ones the first mask lost",
    "lattice_far": "peaks r + 1 apart, decreasing: each is alone in its window by exactly one pixel, every one survives",
}
_NMS_ALL = ((2, 31, 33), (3, 45, 77))      # every content at these two


def nms_cases():
    """-> [(name, shape, content)]: every content at (2, 31, 33) and (3, 45, 77), the plateau map at every shape, the peaks on
    every shape that has rows and columns 31 and 32."""
    out = [(f"{c}-{s[0]}x{s[1]}x{s[2]}", s, c) for s in _NMS_ALL for c in NMS_CONTENTS]
    out += [(f"plateau-{s[0]}x{s[1]}x{s[2]}", s, "plateau") for s in NMS_SHAPES if s not in _NMS_ALL]
    out += [(f"peaks-{s[0]}x{s[1]}x{s[2]}", s, "peaks") for s in ((1, 33, 64), (1, 65, 97))]
    return out


def nms_seam_cases():
    return [c for c in nms_cases() if c[2] == "peaks" and c[1][1] > NMS_TILE and c[1][2] > NMS_TILE]


def lattice_pitch(content: str, radius: int) -> int:
    return radius + 1 if content == "lattice_far" else radius // 2 + 1


def nms_map(shape: Tuple[int, int, int], content: str, radius: int) -> torch.Tensor:
    """fp32 scores [B, h, w] in [0, 2]; only the lattices depend on the radius."""
    B, h, w = shape
    seed = 9300 + 1000 * B + 10 * h + w
    if content == "random":
        return W.uniform(seed, "nms/r", shape, 0.0, 1.0)
    if content == "plateau":
        return torch.floor(W.uniform(seed, "nms/p", shape, 0.0, 8.0)) / 8.0
    if content == "constant":
        return torch.full(shape, 0.375)
    if content == "zeros":
        return torch.zeros(shape)
    if content == "peaks":
        s = W.uniform(seed, "nms/k", shape, 0.0, 0.1)
        single = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (31, 5), (32, 20), (12, 31), (22, 32)]
        for i, (y, x) in enumerate(single):
            if y < h and x < w:
                s[:, y, x] = 1.0 + 0.03125 * i
        for (ya, xa), (yb, xb) in (((31, 40), (32, 40)), ((40, 31), (40, 32))):      # equal pairs across a seam: both are kept
            if yb < h and xb < w:
                s[:, ya, xa] = s[:, yb, xb] = 2.0
        return s
    if content in ("lattice", "lattice_far"):
        p = lattice_pitch(content, radius)
        s = torch.zeros(shape)
        ys, xs = torch.arange(0, h, p), torch.arange(0, w, p)
        n = len(ys) * len(xs)
        rank = torch.arange(n, dtype=torch.float32).reshape(len(ys), len(xs))
        for b in range(B):
            s[b, ::p, ::p] = 1.0 - (rank + b) / (2.0 * (n + B))      # distinct, decreasing in row-major order, in (0.5, 1]
        return s
    raise ValueError(content)


def first_mask_only(scores: torch.Tensor, radius: int) -> torch.Tensor:
    """What simple_nms would return without its two suppression rounds: scores where scores == maxpool(scores)."""
    mp = torch.nn.functional.max_pool2d(scores, kernel_size=2 * radius + 1, stride=1, padding=radius)
    return torch.where(scores == mp, scores, torch.zeros_like(scores))


# ================================================================================================ keypoint selection
CONF_TH = 0.005
SEL_SLABS, SEL_WG, SEL_LDS_K = 64, 1024, 8192
SEL_MAPS = ((8, 8), (9, 11), (40, 56), (61, 67), (96, 128), (120, 160))


@dataclass
class SelCase:
    name: str
    branch: str                           # what the case is there to reach, in words
    nms: torch.Tensor                     # [B, h, w] fp32, non-negative
    k: int                                # max_keypoints
    border: int
    min_kp: int = 0
    fallback_ref: int = 0                 # -1: every frame tests its own count; j >= 0: every frame uses frame j's
    conf_th: float = CONF_TH
    count: Optional[str] = None           # claim on every frame: candidates c "<" | "==" | "==k+1" | ">" relative to k
    low: Optional[Tuple[bool, ...]] = None      # claim per frame: the frame selects at conf_th / 2
    claims: Dict[str, object] = field(default_factory=dict)      # further claims, checked by name in the CPU test


def sel_reference(c: SelCase):
    """oracle/ref_cpu.select_keypoints under the case's fallback rule.  For fallback_ref = j > 0 the batch is rolled so that
    frame j comes first (the reference tests element 0), and the result rolled back."""
    j = c.fallback_ref
    if j <= 0:
        return R.select_keypoints(c.nms, c.conf_th, c.min_kp, c.border, c.k, per_image_fallback=(j < 0))
    B = c.nms.shape[0]
    kps, scs = R.select_keypoints(torch.roll(c.nms, -j, 0), c.conf_th, c.min_kp, c.border, c.k)
    return [kps[(b - j) % B] for b in range(B)], [scs[(b - j) % B] for b in range(B)]


def sel_stats(c: SelCase):
    """Per frame, with numpy and fp32 comparisons (the kernel's arithmetic: th = fp32 conf_th, th / 2 = th * 0.5f):
    cnt_hi (pixels >= conf_th, border ignored), low (the deciding frame's cnt_hi <= min_kp), cand (scores of the candidates in
    row-major order: >= the frame's threshold and inside the border)."""
    a = c.nms.numpy()
    B, h, w = a.shape
    th = np.float32(c.conf_th)
    cnt_hi = [int((a[b] >= th).sum()) for b in range(B)]
    inb = np.zeros((h, w), dtype=bool)
    inb[c.border:max(h - c.border, c.border), c.border:max(w - c.border, c.border)] = True
    out = []
    for b in range(B):
        ref = b if c.fallback_ref < 0 else c.fallback_ref
        low = cnt_hi[ref] <= c.min_kp
        t = th * np.float32(0.5) if low else th
        out.append(dict(cnt_hi=cnt_hi[b], low=low, cand=a[b][(a[b] >= t) & inb]))
    return out


def tie_split(cand: np.ndarray, k: int):
    """For c > k candidates (row-major): (n_gt, n_eq, take_eq, positions of the tie group in the candidate list)."""
    kth = np.sort(cand)[::-1][k - 1]
    n_gt, eq = int((cand > kth).sum()), np.nonzero(cand == kth)[0]
    return n_gt, len(eq), k - n_gt, eq


def _u(seed: int, name: str, B: int, hw: Tuple[int, int], lo: float = 0.01, hi: float = 1.0) -> torch.Tensor:
    return W.uniform(seed, name, (B,) + hw, lo, hi)


def _levels(seed: int, name: str, B: int, hw: Tuple[int, int], n: int) -> torch.Tensor:
    """(randint(0, n) + 1) / 8"""
    return (torch.floor(W.uniform(seed, name, (B,) + hw, 0.0, float(n))) + 1.0) / 8.0


def _three_bands(seed: int, hw: Tuple[int, int], n_hi: Tuple[int, ...], border: int) -> torch.Tensor:
    """Frames whose pixels fall in three bands: frame b has exactly n_hi[b] pixels in [2 conf_th, 1) — the first four of them
    in the border strip, which the fallback count includes and the candidates do not —, every fourth other pixel in
    [0.6, 0.9] * conf_th (a candidate only after the fallback) and the rest below conf_th / 2."""
    h, w = hw
    B = len(n_hi)
    mid = _u(seed, "sel/mid", B, hw, 0.6 * CONF_TH, 0.9 * CONF_TH)
    lowv = _u(seed, "sel/low", B, hw, 0.0, 0.4 * CONF_TH)
    pick = torch.floor(W.uniform(seed, "sel/pick", (B, h, w), 0.0, 4.0)) == 0
    s = torch.where(pick, mid, lowv)
    hi = _u(seed, "sel/hi", B, hw, 2 * CONF_TH, 1.0)
    order = torch.argsort(W.uniform(seed, "sel/ord", (B, h * w)), dim=1, stable=True)
    ys, xs = torch.arange(h).view(h, 1).expand(h, w).reshape(-1), torch.arange(w).view(1, w).expand(h, w).reshape(-1)
    inside = ((ys >= border) & (ys < h - border) & (xs >= border) & (xs < w - border))
    for b in range(B):
        o = order[b]
        strip, inner = o[~inside[o]], o[inside[o]]
        n_strip = min(4, n_hi[b], len(strip))
        idx = torch.cat([strip[:n_strip], inner[:n_hi[b] - n_strip]])
        s[b].view(-1)[idx] = hi[b].view(-1)[idx]
    return s.contiguous()


def _prev(x: np.float32) -> np.float32:
    return np.nextafter(np.float32(x), np.float32(0.0))


def sel_cases():
    """The selection sweep.  Builders compute nothing with the reference; the CPU test checks every claim against it."""
    cs = []

    def add(*a, **kw):
        cs.append(SelCase(*a, **kw))

    # ---- count / compaction kernels
    add("tiny-8x8", "fewer pixels than the 64 slabs: slabs of 8 pixels, 56 of them empty; k >= h * w keeps everything",
        _u(1, "sel/a", 1, (8, 8)), k=100, border=0, count="<")
    add("odd-9x11", "99 pixels (not a multiple of 8) in rows of 11: the last thread's run of 8 ends early, runs cross row ends",
        _u(2, "sel/b", 2, (9, 11)), k=20, border=0, count=">")
    add("odd-9x11-all", "k = h * w: nothing can exceed the bound", _u(2, "sel/b", 2, (9, 11)), k=99, border=0, count="==")
    add("odd-9x11-all+5", "k = h * w + 5", _u(2, "sel/b", 2, (9, 11)), k=104, border=0, count="<")
    add("border-all-8x8", "border = h // 2 = 4 on 8 x 8 leaves no pixel", _u(3, "sel/c", 2, (8, 8)), k=10, border=4, count="<",
        claims={"candidates": 0})
    add("border-row-9x11", "border = h // 2 = 4 on 9 x 11 leaves one row of three pixels", _u(4, "sel/d", 1, (9, 11)), k=2,
        border=4, count="==k+1", claims={"candidates": 3})
    # with border 4 a row's first pixel sits at 4 w = 0 or 4 (mod 8): the pixels that follow a row end inside a thread's run of 8
    # are all in the border columns.  Border 3 on rows of 11: row 3 starts at pixel 33, the run 32 .. 39 enters the interior
    add("border-3-9x11", "a run of 8 crosses from the last border row into the first interior row and ends on interior pixels: the "
        "row counter inside the run decides", _u(4, "sel/d3", 2, (9, 11)), k=99, border=3, count="<", claims={"row_cross": True})
    add("border-all-40x56", "border = h // 2 = 20 on 40 x 56 leaves no row", _u(5, "sel/e", 3, (40, 56)), k=64, border=20, count="<",
        claims={"candidates": 0})
    add("border-row-61x67", "border = h // 2 = 30 on 61 x 67 leaves one row of seven pixels", _u(6, "sel/f", 1, (61, 67)), k=3,
        border=30, count=">", claims={"candidates": 7})
    add("rows-40x56", "rows of 56 = 7 runs of 8, three frames, border 4: the aligned case", _u(7, "sel/g", 3, (40, 56)), k=512,
        border=4, count=">")
    add("rows-61x67", "rows of 67, border 4, more candidates than one sweep of 1024 and fewer than k: the row-major copy loops",
        _u(8, "sel/h", 2, (61, 67)), k=4000, border=4, count="<")
    add("empty-40x56", "all zeros: no candidate in any slab", torch.zeros(2, 40, 56), k=100, border=4, min_kp=10, count="<",
        low=(True, True), claims={"candidates": 0})

    # ---- fallback decision (cnt_hi <= min_keypoints), thresholds
    bands = _three_bands(20, (40, 56), (37, 37), 4)
    add("fallback-at-min", "cnt_hi == min_keypoints: <= falls back to conf_th / 2; the count includes border pixels", bands, k=2000,
        border=4, min_kp=37, low=(True, True), claims={"cnt_hi": (37, 37)})
    add("fallback-at-min+1", "cnt_hi == min_keypoints + 1: no fallback", bands, k=2000, border=4, min_kp=36, low=(False, False),
        claims={"cnt_hi": (37, 37)})
    mixed = _three_bands(21, (40, 56), (300, 12, 40), 4)
    add("fallback-per-frame", "fallback_ref = -1: frame 0 stays at conf_th, frames 1 and 2 fall back", mixed, k=2000, border=4, min_kp=40,
        fallback_ref=-1, low=(False, True, True))
    add("fallback-ref-0", "fallback_ref = 0: frame 0 (no fallback) decides for all", mixed, k=2000, border=4, min_kp=40, low=(False,) * 3)
    add("fallback-ref-1", "fallback_ref = 1: frame 1 (fallback) decides for all, frame 0 included", mixed, k=2000, border=4, min_kp=40,
        fallback_ref=1, low=(True,) * 3)
    add("fallback-ref-2", "fallback_ref = 2 at its own count == min_keypoints", mixed, k=150, border=4, min_kp=40, fallback_ref=2,
        low=(True,) * 3)
    th = np.float32(CONF_TH)
    edge = torch.zeros(1, 8, 8)
    edge[0, 1, 1:5] = torch.from_numpy(np.array([th, _prev(th), th * np.float32(0.5), _prev(th * np.float32(0.5))], dtype=np.float32))
    edge[0, 5, 2], edge[0, 6, 6] = 0.25, 0.5
    add("threshold-exact", "scores at conf_th and its predecessor, no fallback: >= keeps the first only", edge, k=64, border=0, min_kp=2,
        low=(False,), claims={"candidates": 3, "kept": (th, 0.25, 0.5)})
    add("threshold-half-exact", "scores at conf_th / 2 and its predecessor after the fallback: >= keeps the first only", edge, k=64,
        border=0, min_kp=3, low=(True,), claims={"candidates": 5, "kept": (th, _prev(th), th * np.float32(0.5), 0.25, 0.5)})

    # ---- c against k
    one = torch.where(W.uniform(30, "sel/sp", (1, 40, 56)) < -0.5, _u(30, "sel/sv", 1, (40, 56)), torch.zeros(1, 40, 56))
    sparse = torch.cat([one, torch.flip(one, [1, 2])]).contiguous()      # the mirrored frame has the same number inside the border
    c_eq = int((one[0, 4:-4, 4:-4] > 0).sum())
    add("c==k", "exactly k candidates: <= keeps the row-major order, nothing is sorted", sparse, k=c_eq, border=4, count="==")
    add("c==k+1", "one candidate more than k: the smallest score is dropped, the rest sorted", sparse, k=c_eq - 1, border=4, count="==k+1")
    add("k=1", "k = 1: the radix select ends on the maximum, a sort of one key", _u(31, "sel/k1", 2, (9, 11)), k=1, border=0, count=">")
    add("k=1024", "k = the workgroup width", _u(32, "sel/w", 2, (61, 67)), k=1024, border=4, count=">")
    add("k=1025", "k = the workgroup width + 1: every strided loop takes a second trip", _u(32, "sel/w", 2, (61, 67)), k=1025, border=4,
        count=">")
    add("k=8192", "the largest bound sorted in LDS", _u(33, "sel/x", 2, (120, 160)), k=8192, border=4, count=">")
    add("k=8193-global", "global-memory sort, bound not a power of two (padded to 16384)", _u(34, "sel/y", 1, (96, 128)), k=8193,
        border=4, count=">", claims={"global_sort": True})
    add("k=10000-global", "global-memory sort, bound not a power of two, two frames of the largest map", _u(33, "sel/x", 2, (120, 160)),
        k=10000, border=4, count=">", claims={"global_sort": True})
    add("k=8193-global-ties", "global-memory sort with a tie group cut by the bound", _levels(35, "sel/z", 1, (96, 128), 4), k=8193,
        border=4, count=">", claims={"global_sort": True})
    add("k=h*w-96x128", "k = h * w = 12288 > 8192: keep-all takes the LDS kernel and never sorts", _u(34, "sel/y", 1, (96, 128)),
        k=96 * 128, border=0, count="==")

    # ---- ties and the radix passes
    add("tie-straddle", "the k-th score's tie group spreads over all 1024-candidate chunks, the cut falls inside one",
        _levels(40, "sel/t", 1, (61, 67), 4), k=1500, border=4, count=">", claims={"straddle": True})
    add("all-equal", "every candidate equal: each radix pass lands in one bin, the lowest indices are taken",
        torch.full((2, 61, 67), 0.5), k=1024, border=4, count=">", claims={"all_equal": True})
    bits = (torch.floor(W.uniform(41, "sel/lb", (2, 40, 56), 0.0, 256.0)).to(torch.int32) + 0x3E800000)
    add("low-byte", "scores that differ in their lowest byte only: three radix passes in one bin, the last one decides",
        bits.view(torch.float32).contiguous(), k=700, border=4, count=">", claims={"low_byte": True})
    return cs


def sel_regime_batch():
    """Three frames in different regimes for the batch-equals-alone test: c <= k, c > k, empty."""
    a = torch.where(W.uniform(50, "sel/ra", (1, 40, 56)) < -0.8, _u(50, "sel/rv", 1, (40, 56)), torch.zeros(1, 40, 56))
    return SelCase("regimes", "frames with c <= k, c > k and no candidate in one batch, each under its own fallback test",
                   torch.cat([a, _u(51, "sel/rb", 1, (40, 56)), torch.zeros(1, 40, 56)]).contiguous(), k=300, border=4, min_kp=10,
                   fallback_ref=-1, low=(False, False, True))


# ================================================================================================ score lookup
LOOKUP_GUARD = 320      # rows of sentinel on each side of kpts / out (the launch covers up to 255 rows past n_max)
