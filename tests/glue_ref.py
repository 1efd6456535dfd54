"""Plain restatements of the small kernels between the models (csrc/extras.hip, csrc/adagml.hip, the sampling tail of
csrc/sfd2_post.hip), for tests/test_gpu_glue_kernels.py, and the seeded cases that file and tests/test_glue_ref_cpu.py share.

Written from the reference lines the kernels' header comments cite: the recogniser epilogue (localization/frame.py:96-121), the
full descending sort and the landmark vote (localization/multimap3d.py:348-379), nearest-neighbour top-2
(localization/matchers/nearest_neighbor.py:5-17), projection refinement (localization/singlemap3d.py:405-433), AdaGML pruning,
stopping and result scatter (nets/adagml.py:354-372, 382-396, 516-531) and descriptor sampling (nets/sfd2.py:53-64).  Host code
over numpy / CPU torch, float64 wherever anything is floating point, loops where they are clearest.  Nothing here calls the
library under test; the case builders use its seeded input generators (pram_amd.weights) only."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from pram_amd import weights as W

GAP = 1e-3        # top-2 cases: least distance between best / second / third of a row that is not a planted tie
MARGIN = 1e-4     # threshold cases: least distance of a confidence that is not a planted tie from its threshold


# ================================================================================================ references
def row_top2(x, largest: bool, n_valid=None, row_lens=None, col_lens=None):
    """x [B, M, ld] -> (best [B, M], second [B, M], index of best int64 [B, M]) over the first n columns of the first m rows of
    every set (m = row_lens[b] or M, n = col_lens[b] or n_valid or ld).  Ties go to the lowest index; the second value is the
    second element of the sorted row (equal to the best when the best is duplicated), -inf / +inf (largest / smallest) when
    there is none.  Rows that are not computed hold (0, 0, -1)."""
    x = np.asarray(x, dtype=np.float64)
    B, M, ld = x.shape
    v0, v1, i0 = np.zeros((B, M)), np.zeros((B, M)), np.full((B, M), -1, dtype=np.int64)
    none = -np.inf if largest else np.inf
    for b in range(B):
        m = M if row_lens is None else int(row_lens[b])
        n = (n_valid or ld) if col_lens is None else int(col_lens[b])
        for r in range(m):
            row = x[b, r, :n]
            order = sorted(range(n), key=lambda j: ((-row[j] if largest else row[j]), j))
            v0[b, r] = row[order[0]] if n > 0 else none
            v1[b, r] = row[order[1]] if n > 1 else none
            i0[b, r] = order[0] if n > 0 else -1
    return v0, v1, i0


def proj_dist(sim, kpts, uv, rng: float, n: int):
    """dist [M, n] float64 = sqrt(2 - 2 sim + 1e-6) + (100 where ||kpt_i - uv_j|| >= rng) (singlemap3d.py:424-431)."""
    sim = np.asarray(sim, dtype=np.float64)[:, :n]
    kpts, uv = np.asarray(kpts, dtype=np.float64), np.asarray(uv, dtype=np.float64)[:, :n]
    err = np.sqrt((kpts[:, 0:1] - uv[0][None]) ** 2 + (kpts[:, 1:2] - uv[1][None]) ** 2)
    d = np.sqrt(2.0 - 2.0 * sim + 1e-6)
    return d + np.where(err >= rng, 100.0, 0.0)


def proj_dist_top2(sim, kpts, uv, rng: float, n: int):
    """-> (d0 [M], d1 [M], i0 int64 [M]): the two smallest distances of every row and the index of the smallest (lowest index on
    ties); d1 = +inf when n = 1 (singlemap3d.py:432)."""
    d = proj_dist(sim, kpts, uv, rng, n)
    v0, v1, i0 = row_top2(d[None], False)
    return v0[0], v1[0], i0[0]


def project_points(xyz, K, Tcw, im_w: float, im_h: float):
    """-> (uvd [3, N] float64 = u, v, depth of every point, mask bool [N], keep int64 [count]) (singlemap3d.py:405-415)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    K, T = np.asarray(K, dtype=np.float64), np.asarray(Tcw, dtype=np.float64)
    n = xyz.shape[0]
    uvd, mask = np.zeros((3, n)), np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            c = T[:3, :3] @ xyz[i] + T[:3, 3]
            p = K @ c
            u, v = np.float64(p[0]) / np.float64(p[2]), np.float64(p[1]) / np.float64(p[2])
            uvd[:, i] = (u, v, p[2])
            mask[i] = (p[2] > 0) and (p[2] < 100) and (u >= 0) and (u < im_w) and (v >= 0) and (v < im_h)
    return uvd, mask, np.nonzero(mask)[0]


def seg_epilogue(logits, lens, thr: float):
    """logits [B, N, C] -> (seg ids int32 [B, N] = first arg-max - 1, non-background mask int32 [B, N] = softmax[0] < thr,
    n_non_bg int32 [B], softmax float64 [B, N, C]); rows at and beyond lens[b] hold (-2, 0, zeros) (frame.py:101-121)."""
    x = np.asarray(logits, dtype=np.float64)
    B, N, C = x.shape
    ids, mask, sc = np.full((B, N), -2, dtype=np.int32), np.zeros((B, N), dtype=np.int32), np.zeros((B, N, C))
    for b in range(B):
        for n in range(N if lens is None else int(lens[b])):
            e = np.exp(x[b, n] - x[b, n].max())
            sc[b, n] = e / e.sum()
            ids[b, n] = int(np.argmax(x[b, n])) - 1
            mask[b, n] = int(sc[b, n, 0] < thr)
    return ids, mask, mask.sum(1).astype(np.int32), sc


def row_sort_desc(x):
    """-> (values, indices int64) of every row sorted by value descending, equal values (+0.0 and -0.0 are equal) in ascending
    index order: torch.topk(k = C) made canonical (multimap3d.py:348-350)."""
    x = np.asarray(x)
    idx = np.stack([np.array(sorted(range(x.shape[1]), key=lambda j: (-float(r[j]), j)), dtype=np.int64) for r in x]) \
        if x.shape[0] else np.zeros(x.shape, dtype=np.int64)
    return np.take_along_axis(x, idx, 1), idx


def seg_vote(sorted_ids, sorted_vals, topk: int):
    """The vote of multimap3d.py:351-379 over every token's classes sorted by score ([n, C] each): rank k = 0, 1, ...: the classes
    at sorted position k that are not background (0) and were not seen at an earlier rank, most tokens first (equal counts in
    ascending class id), until topk are collected.  -> [(class id, rank, token ids ascending, float64 mean of the rank-k scores)]."""
    ids, vals = np.asarray(sorted_ids), np.asarray(sorted_vals, dtype=np.float64)
    n, c = ids.shape
    out, used = [], set()
    for k in range(c):
        count = {}
        for t in range(n):
            count[int(ids[t, k])] = count.get(int(ids[t, k]), 0) + 1
        cand = sorted((s for s in count if s != 0 and s not in used), key=lambda s: (-count[s], s))
        used.update(count)
        for s in cand:
            tok = np.nonzero(ids[:, k] == s)[0]
            out.append((s, k, tok, float(np.mean(vals[tok, k]))))
            if len(out) >= topk:
                return out
    return out


def adagml_prune(logit, thr: float, n_min: int, lens_in, T: int):
    """logit [S, T] -> per set: the surviving token ids in order (all of them when the set has fewer than n_min tokens), the
    number of confidences below thr, the float64 confidences (adagml.py:354-365, 527-529)."""
    lg = np.asarray(logit, dtype=np.float64)
    keep, below, conf = [], [], np.zeros(lg.shape)
    for s in range(lg.shape[0]):
        n = T if lens_in is None else int(lens_in[s])
        c = 1.0 / (1.0 + np.exp(-lg[s, :n]))
        conf[s, :n] = c
        keep.append(np.nonzero(c > thr)[0] if n >= n_min else np.arange(n))
        below.append(int(np.sum(c < thr)))
    return keep, np.array(below, dtype=np.int32), conf


def stop_value(below0: int, below1: int, num_points: float) -> float:
    """check_if_stop's quantity (adagml.py:529): a pair stops when it exceeds 0.95."""
    return 1.0 - float(below0 + below1) / float(num_points)


def adagml_layer_state(st: dict, lens_new, n_below, ind, layer: int, last: bool) -> dict:
    """One layer of the per-pair loop of adagml.py:352-380 for B pairs.  st: active [B], lens [2B] (side 0 then side 1), tiny [B],
    stop_layer [B], lens_final [2B], ind_final [2B, T], num_points [B]; lens_new / n_below [2B] from the pruning of this layer
    or None on the first.  -> the new state, plus lens_stop (the lengths of the pairs that stop here, else 0) and lens_eff (the
    lengths of the pairs that go on, else 0).  An inactive pair ignores everything."""
    B = len(st["active"])
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    out["lens_stop"], out["lens_eff"] = np.zeros(2 * B, dtype=np.int32), np.zeros(2 * B, dtype=np.int32)
    for b in range(B):
        if not st["active"][b]:
            continue
        l0, l1 = int(st["lens"][b]), int(st["lens"][B + b])
        stop = False
        if lens_new is not None:
            l0, l1 = int(lens_new[b]), int(lens_new[B + b])
            if l0 <= 5 or l1 <= 5:
                out["tiny"][b] = 1
            stop = stop_value(int(n_below[b]), int(n_below[B + b]), st["num_points"][b]) > 0.95
        if last:
            stop = True
        out["lens"][b], out["lens"][B + b] = l0, l1
        if stop:
            out["active"][b], out["stop_layer"][b] = 0, layer
            for s, l in ((b, l0), (B + b, l1)):
                out["lens_stop"][s] = out["lens_final"][s] = l
                out["ind_final"][s] = np.asarray(ind)[s]
        else:
            out["lens_eff"][b], out["lens_eff"][B + b] = l0, l1
    return out


def adagml_scores4(col_self: torch.Tensor, col_cross: torch.Tensor) -> torch.Tensor:
    """[S, T] self / cross attention scores -> [S * T, 4] rows (self, cross, 0, 0): the pooling head's input (adagml.py:348-351),
    padded to four columns."""
    z = torch.zeros(col_self.numel(), dtype=col_self.dtype)
    return torch.stack([col_self.reshape(-1), col_cross.reshape(-1), z, z], 1)


def adagml_scatter(matches0, mscores0, ind0, ind1, lens0, m_full: int):
    """matches_full[ind0[i]] = ind1[matches0[i]] (valid matches only), scores_full[ind0[i]] = mscores0[i] (adagml.py:382-393)."""
    m0, ms0 = np.asarray(matches0), np.asarray(mscores0)
    B, T = m0.shape
    om, osc = np.full((B, m_full), -1, dtype=np.int64), np.zeros((B, m_full), dtype=ms0.dtype)
    for b in range(B):
        for i in range(T if lens0 is None else int(lens0[b])):
            row = int(ind0[b][i])
            osc[b, row] = ms0[b, i]
            if m0[b, i] >= 0:
                om[b, row] = int(ind1[b][int(m0[b, i])])
    return om, osc


def sample_grid(kpts: torch.Tensor, fh: int, fw: int, s: int) -> torch.Tensor:
    """The coordinate map of sample_descriptors (nets/sfd2.py:53-64), in the keypoints' own float32 like the reference:
    u = ((k - s/2 + 0.5) / (w s - s/2 - 0.5, h s - s/2 - 0.5)) * 2 - 1; s = 0: the keypoints are grid coordinates already."""
    if s <= 0:
        return kpts
    k = kpts - s / 2 + 0.5
    k = k / torch.tensor([fw * s - s / 2 - 0.5, fh * s - s / 2 - 0.5], dtype=k.dtype)
    return k * 2 - 1


def sample_nhwc(fmap: torch.Tensor, kpts: torch.Tensor, lens, s: int, l2norm: bool) -> torch.Tensor:
    """fmap [B, fh, fw, C], kpts [B, N, 2] -> float64 [B, N, C]: F.grid_sample(bilinear, align_corners, zero padding) in float64
    at the reference's grid coordinates, F.normalize over the channels; rows at and beyond lens[b] are zero."""
    B, fh, fw, C = fmap.shape
    g = sample_grid(kpts, fh, fw, s).double()
    d = F.grid_sample(fmap.double().permute(0, 3, 1, 2), g[:, None], mode="bilinear", align_corners=True)[:, :, 0].permute(0, 2, 1)
    if l2norm:
        d = F.normalize(d, p=2, dim=2)
    d = d.clone()
    if lens is not None:
        for b in range(B):
            d[b, int(lens[b]):] = 0
    return d


def score_lookup(score_map: torch.Tensor, kpts: torch.Tensor, lens) -> torch.Tensor:
    """score_map [Bm, H, W] (Bm = 1: one map for every set), kpts [B, N, 2] -> scores[b, n] = map[b][int(y)][int(x)]."""
    B, N = kpts.shape[:2]
    out = torch.zeros(B, N, dtype=score_map.dtype)
    for b in range(B):
        for n in range(N if lens is None else int(lens[b])):
            out[b, n] = score_map[b if score_map.shape[0] > 1 else 0, int(kpts[b, n, 1]), int(kpts[b, n, 0])]
    return out


def l2norm_rows(x: torch.Tensor) -> torch.Tensor:
    return F.normalize(x.double(), p=2, dim=-1, eps=1e-12)


def resize_bilinear(x: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    return F.interpolate(x.double(), size=(oh, ow), mode="bilinear", align_corners=True)


# ================================================================================================ seeded cases
def perm_rows(seed: int, name: str, rows: int, n: int) -> torch.Tensor:
    """int64 [rows, n]: a permutation of 0 .. n-1 per row."""
    return torch.argsort(W.uniform(seed, name, (rows, n)), dim=1, stable=True)


def spaced(seed: int, name: str, rows: int, n: int, lo: float, hi: float) -> torch.Tensor:
    """float32 [rows, n] in (lo, hi): per row a shuffled n-point grid plus a jitter of at most a quarter of its spacing, so any
    two values of a row are at least half a spacing (hi - lo) / n apart."""
    step = (hi - lo) / max(n, 1)
    g = perm_rows(seed, name + "/p", rows, n).double() + 0.5 + 0.25 * W.uniform(seed, name + "/j", (rows, n)).double()
    return (lo + g * step).float()


def garbage(seed: int, name: str, shape) -> torch.Tensor:
    """NaN-free values of magnitude up to 1e30 and both signs: what an unmasked padding column would contribute."""
    return W.uniform(seed, name, tuple(shape)) * 1e30


def sorted_gaps(values) -> tuple:
    """(best - second, second - third) of the ascending-sorted values (inf where there is no such pair)."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    return (v[1] - v[0] if v.size > 1 else np.inf), (v[2] - v[1] if v.size > 2 else np.inf)


# ---- row_top2
TOP2_LD, TOP2_B = 72, 3
TOP2_N, TOP2_M = (1, 2, 63, 64, 65, 70), (1, 5)
TOP2_RAGGED = (([5, 0, 3], [70, 9, 1]), ([2, 5, 1], [0, 2, 64]))      # (row_lens, col_lens); the second has an empty set of columns


def top2_case(M: int, n: int, largest: bool) -> dict:
    """x [3, M, 72]: n valid columns spaced in (-1, 1), garbage beyond.  With M = 5 set 0 carries the planted rows (as far as n
    allows): row 0 the best value twice, at columns 3 and 67 (one lane, two loop passes); row 1 twice at columns 5 and 6 (two
    lanes); row 2 the two best at columns 4 and 68 (one lane), the rest far away; row 3 constant.  `ties`: rows whose best is
    duplicated on purpose."""
    seed = 1000 + 10 * n + M
    x = garbage(seed, "top2/g", (TOP2_B, M, TOP2_LD))
    x[:, :, :n] = spaced(seed, "top2/v", TOP2_B * M, n, -1.0, 1.0).view(TOP2_B, M, n)
    sg = 1.0 if largest else -1.0
    ties = set()
    if M == 5:
        if n >= 69:
            x[0, 0, 3] = x[0, 0, 67] = 2.0 * sg
            x[0, 2, 4], x[0, 2, 68] = 2.0 * sg, 1.5 * sg
            ties.add((0, 0))
        if n >= 7:
            x[0, 1, 5] = x[0, 1, 6] = 2.0 * sg
            ties.add((0, 1))
        x[0, 3, :n] = 0.25
        ties.add((0, 3))
    return {"x": x.contiguous(), "n": n, "ties": ties}


# ---- projection top-2
PROJ_M, PROJ_N, PROJ_RANGE, PROJ_PAD = (1, 6), (1, 2, 65, 130), 5.0, 7


def proj_case(M: int, n: int) -> dict:
    """sim [M, (n+3)//4*4] spaced in (-0.9, 0.8) with garbage in the pad; integer pixel coordinates in [0, 12)^2, so the pixel
    error and its `>= range` test are exact in float32 and float64 alike; uv64 [2, n + 7] float64 with far-away pad columns.
    With M = 6 (as far as n allows): row 0 duplicates its best column (sim 0.9, same uv, error 0) at columns 3 and 67, row 1 at
    columns 5 and 6 (0 and 1 when n < 7); row 2 sits 100 px away from everything (every column penalised); row 3's best column
    by far (sim 0.9) lies at pixel distance exactly `range` — (5, 5) against (8, 9) — and must be penalised."""
    seed = 2000 + 10 * n + M
    ld = (n + 3) // 4 * 4
    sim = garbage(seed, "proj/g", (M, ld))
    sim[:, :n] = spaced(seed, "proj/s", M, n, -0.9, 0.8)
    kpts = torch.floor(W.uniform(seed, "proj/k", (M, 2), 0.0, 12.0))
    uv = torch.floor(W.uniform(seed, "proj/uv", (2, n), 0.0, 12.0))
    ties, exact_col = set(), None
    if M == 6:
        if n >= 68:
            uv[:, 67] = uv[:, 3]
            kpts[0] = uv[:, 3]
            sim[0, 3] = sim[0, 67] = 0.9
            ties.add(0)
        if n >= 2:
            a, b = (5, 6) if n >= 7 else (0, 1)
            uv[:, b] = uv[:, a]
            kpts[1] = uv[:, a]
            sim[1, a] = sim[1, b] = 0.9
            ties.add(1)
        kpts[2] = torch.tensor([100.0, 100.0])
        exact_col = 9 if n >= 10 else (0 if n == 1 else None)      # n = 2: both columns are the planted pair
        if exact_col is not None:
            kpts[3] = torch.tensor([5.0, 5.0])
            uv[:, exact_col] = torch.tensor([8.0, 9.0])
            sim[3, exact_col] = 0.9
    uv64 = torch.full((2, n + PROJ_PAD), 1e4, dtype=torch.float64)
    uv64[:, :n] = uv.double()
    return {"sim": sim.contiguous(), "kpts": kpts.contiguous(), "uv": uv.contiguous(), "uv64": uv64.contiguous(), "n": n,
            "ties": ties, "exact_col": exact_col}


# ---- projection of map points
PP_W, PP_H = 128.0, 96.0
PP_K = np.array([[128.0, 0.0, 64.0], [0.0, 128.0, 48.0], [0.0, 0.0, 1.0]])
PP_N = (0, 1, 1023, 1024, 1025, 2500)


def _pp_pose():
    a = 0.3
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    T[:3, 3] = (0.5, -0.25, 2.0)
    return T


def pp_case(n: int, kind: str = "half") -> dict:
    """n map points in front of a rotated, shifted camera: `half` about half of them in the frustum, `inside` all, `outside`
    none (behind the camera)."""
    seed = 3000 + n
    T = _pp_pose()
    spread = {"half": 0.7, "inside": 0.3, "outside": 0.3}[kind]
    cam = torch.stack([W.uniform(seed, "pp/x", (n,)).double() * spread, W.uniform(seed, "pp/y", (n,)).double() * spread * 0.75,
                       W.uniform(seed, "pp/z", (n,), 1.5, 3.0).double() * (-1.0 if kind == "outside" else 1.0)], 1).numpy()
    cam[:, :2] *= np.abs(cam[:, 2:3])                                    # camera-frame points -> world
    xyz = (cam - T[:3, 3]) @ T[:3, :3]
    return {"xyz": xyz.reshape(n, 3), "K": PP_K, "T": T, "w": PP_W, "h": PP_H}


def pp_boundary_case() -> dict:
    """Identity pose, K = (f 128, c (64, 48)), a 128 x 96 image: every product below is exact in float64.  Points on each edge of
    the keep test, in this order, with the expected decision."""
    pts = [((-0.5, 0.0, 1.0), True),        # u = 0: kept
           ((0.5, 0.0, 1.0), False),        # u = im_w: dropped
           ((0.0, -0.375, 1.0), True),      # v = 0: kept
           ((0.0, 0.375, 1.0), False),      # v = im_h: dropped
           ((1.0, 1.0, 0.0), False),        # depth 0: dropped (u = v = inf)
           ((0.0, 0.0, 100.0), False),      # depth 100: dropped
           ((0.0, 0.0, 99.5), True),
           ((0.25, 0.25, 2.0), True),
           ((0.0, 0.0, -1.0), False)]
    return {"xyz": np.array([p for p, _ in pts]), "K": PP_K, "T": np.eye(4), "w": PP_W, "h": PP_H,
            "expect": np.array([k for _, k in pts])}


# ---- recogniser epilogue
SEG_B, SEG_N, SEG_C, SEG_THR = 3, (1, 16, 17, 37), (2, 63, 64, 65, 113), 0.2


def seg_tie_classes(C: int):
    return (3, 70) if C > 70 else ((1, C - 1) if C >= 3 else (0, 1))


def seg_case(N: int, C: int) -> dict:
    """logits [3, N, C]; set 0 carries the planted rows (as far as N allows): row 0 an arg-max tie between two classes in
    different lanes (3 and 70 when C allows), row 1 a background logit far above the rest (softmax[0] ~ 1), row 2 far below."""
    seed = 4000 + 10 * C + N
    x = W.normal(seed, "seg/l", (SEG_B, N, C), 2.0)
    x[:, :, 0] += 1.0
    a, b = seg_tie_classes(C)
    x[0, 0, a] = x[0, 0, b] = 9.0
    if N >= 3:
        x[0, 1, 0], x[0, 2, 0] = 20.0, -20.0
    return {"x": x.contiguous(), "lens": [N, 0, min(5, N)], "tie": (a, b)}


# ---- sort
SORT_COLS = (1, 2, 3, 255, 256, 257, 1023, 1024)


def sort_case(cols: int) -> torch.Tensor:
    """[3, cols]: a quantised row (many exact ties), one with +inf and -inf in it, a constant row."""
    x = torch.floor(W.normal(5000 + cols, "sort/x", (3, cols), 3.0))
    if cols >= 3:
        x[1, cols // 2], x[1, 0] = float("inf"), float("-inf")
    x[2] = -1.5
    return x.contiguous()


def sort_zero_case() -> torch.Tensor:
    """Rows mixing +0.0 and -0.0 with other values: the two zeros are equal and keep their index order."""
    short = torch.tensor([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, -0.0, 2.0])
    x = torch.floor(W.normal(5999, "sort/z", (2, 300), 1.0))
    x[0] = torch.where(x[0] == 0, torch.where(torch.arange(300) % 2 == 0, torch.tensor(-0.0), torch.tensor(0.0)), x[0])
    x[1, :9] = short
    return x.contiguous()


# ---- landmark vote
VOTE_CASES = ((0, 5, 3), (1, 2, 4), (70, 9, 3), (1030, 17, 40), (64, 1024, 5))


def _vote_ids(seed: int, n: int, C: int, col0, col1=None) -> torch.Tensor:
    """int64 [n, C]: per token a permutation of the classes with col0[t] at rank 0 and (if given) col1[t] at rank 1."""
    ids = perm_rows(seed, "vote/p", n, C)
    for t in range(n):
        row = [int(v) for v in ids[t]]
        front = [int(col0[t])] + ([int(col1[t])] if col1 is not None else [])
        assert len(set(front)) == len(front)
        ids[t] = torch.tensor(front + [v for v in row if v not in front])
    return ids


def _spread(seed: int, counts: dict, n: int) -> list:
    """a list of n class ids with the given multiplicities, shuffled"""
    flat = [c for c, k in counts.items() for _ in range(k)]
    assert len(flat) == n, (len(flat), n)
    return [flat[int(i)] for i in perm_rows(seed, "vote/s", 1, n)[0]]


def vote_case(n: int, C: int, topk: int, variant: int = 0) -> dict:
    """Sorted class lists built as permutations (not from scores), so that the ranks can be planted:
    (1, 2, 4): one token, landmark 1 first -> one winner, fewer than topk.
    (70, 9, 3): rank 0 = background 30 tokens (most frequent, skipped), landmarks 2 and 4 with 12 each (a tie: 2 first), 7 with 9,
      5 with 7: topk fills in the middle of rank 0 and landmark 5, seen there, is not selected.  `variant` relabels the landmarks.
      (The vote ends where topk fills, so a landmark that was seen but not selected can never come up again at a later rank:
      "every class seen becomes used" and "only the winners become used" give the same output on every input, and no case here or
      anywhere can tell them apart.)
    (1030, 17, 40): rank 0 = background 200, landmarks 1 .. 13 with 51 .. 63 tokens, 14 with 89; landmarks 15 and 16
      appear at rank 1 only (120 and 80 tokens): 16 winners for topk = 40, tokens beyond 1024.
    (64, 1024, 5): the class limit; rank 0 = background 20, landmarks 1023, 512, 1, 700 with 15, 11, 10, 8; rank 1 = landmark 3 (49
      tokens) and the already used 1023."""
    seed = 6000 + n + 7 * variant
    col1 = None
    if n == 0:
        ids = torch.zeros(0, C, dtype=torch.int64)
    elif (n, C) == (1, 2):
        ids = _vote_ids(seed, n, C, [1])
    elif (n, C) == (70, 9):
        lab = [[2, 4, 7, 5], [1, 8, 3, 6], [3, 5, 2, 8]][variant]
        ids = _vote_ids(seed, n, C, _spread(seed, {0: 30, lab[0]: 12, lab[1]: 12, lab[2]: 9, lab[3]: 7}, n))
    elif (n, C) == (1030, 17):
        counts = {0: 200, **{j: 50 + j for j in range(1, 15)}}
        counts[14] += n - sum(counts.values())
        col0 = _spread(seed, counts, n)
        second = iter(_spread(seed + 1, {15: 120, 16: 80}, 200))
        col1 = [next(second) if c == 0 else 0 for c in col0]
        ids = _vote_ids(seed, n, C, col0, col1)
    elif (n, C) == (64, 1024):
        col0 = _spread(seed, {0: 20, 1023: 15, 512: 11, 1: 10, 700: 8}, n)
        col1 = [3 if c == 1023 else 1023 for c in col0]
        for i in [i for i, c in enumerate(col0) if c != 1023][:34]:
            col1[i] = 3
        ids = _vote_ids(seed, n, C, col0, col1)
    else:
        raise ValueError((n, C))
    vals = torch.sort(W.uniform(seed, "vote/v", (n, C), 0.0, 1.0), dim=1, descending=True).values
    return {"ids": ids.contiguous(), "vals": vals.contiguous(), "topk": topk}


def vote_segs(case: dict) -> np.ndarray:
    """the [n, C] score matrix whose descending sort gives the case's class lists (the scores of a row are distinct)"""
    ids, vals = case["ids"].numpy(), case["vals"].numpy()
    segs = np.zeros(ids.shape, dtype=np.float32)
    np.put_along_axis(segs, ids, vals, 1)
    return segs


# ---- AdaGML pruning
PRUNE_S, PRUNE_T, PRUNE_LDX, PRUNE_NMIN = 4, (40, 1030, 2050), 256, 8
PRUNE_KINDS = ("random", "all", "none", "last", "tie")
PRUNE_SEED = {40: 7100, 1030: 7102, 2050: 7109}      # seeds whose confidences keep MARGIN from both thresholds (test_glue_ref_cpu.py)


def prune_lens(T: int):
    return [T, T - 1, 7, 0]


def prune_state(T: int) -> dict:
    """x [4, T, 256], cos / sin [4, T, 32] with a different value at every (set, row, column), exact in float32; ind [4, T]: a
    permutation per set."""
    row = torch.arange(PRUNE_S * T, dtype=torch.float32).view(PRUNE_S, T, 1)
    x = row + torch.arange(PRUNE_LDX, dtype=torch.float32) / 1024.0
    cos = -row - torch.arange(32, dtype=torch.float32) / 64.0
    sin = 2.0 * row + torch.arange(32, dtype=torch.float32) / 64.0 + 0.5
    ind = perm_rows(7000 + T, "prune/ind", PRUNE_S, T).to(torch.int32)
    return {"x": x.contiguous(), "cos": cos.contiguous(), "sin": sin.contiguous(), "ind": ind.contiguous()}


def prune_logits(T: int, kind: str):
    """-> (logit [4, T], thr).  random: N(0, 2^2) against 0.55; all / none: +-10; last: -10 but for the last three tokens of every
    set (the last 1024-token chunk when T > 1024); tie: thr = 0.5 and every third logit exactly 0 (sigmoid = 0.5 exactly in
    float32: 1 / (1 + 1)), which is neither kept nor counted below."""
    lg = W.normal(PRUNE_SEED[T] + T, "prune/l", (PRUNE_S, T), 2.0)
    if kind == "random":
        return lg, 0.55
    if kind == "all":
        return torch.full_like(lg, 10.0), 0.55
    if kind == "none":
        return torch.full_like(lg, -10.0), 0.55
    if kind == "last":
        lg = torch.full_like(lg, -10.0)
        for s, n in enumerate(prune_lens(T)):
            lg[s, max(n - 3, 0):n] = 10.0
        return lg, 0.55
    assert kind == "tie"
    lg[:, ::3] = 0.0
    return lg, 0.5


def prune_logits4(lg: torch.Tensor) -> torch.Tensor:
    """[S * T, 4]: the logits in column 0, values that would decide differently in the others."""
    f = lg.reshape(-1)
    return torch.stack([f, -f, torch.full_like(f, 100.0), torch.full_like(f, -100.0)], 1).contiguous()


# ---- AdaGML layer state
LS_B, LS_T = 3, 40


def layer_state_init() -> dict:
    """Three pairs: 0 and 1 running, 2 stopped at layer 1 already (its final lengths and ids must never change)."""
    ind_final = np.full((2 * LS_B, LS_T), -7, dtype=np.int32)
    ind_final[2], ind_final[5] = 100 + np.arange(LS_T), 200 + np.arange(LS_T)
    return {"active": np.array([1, 1, 0], dtype=np.int32), "lens": np.array([40, 38, 35, 40, 37, 33], dtype=np.int32),
            "tiny": np.zeros(LS_B, dtype=np.int32), "stop_layer": np.array([-1, -1, 1], dtype=np.int32),
            "lens_final": np.array([0, 0, 35, 0, 0, 33], dtype=np.int32), "ind_final": ind_final,
            "num_points": np.array([80.0, 75.0, 68.0], dtype=np.float32)}


def layer_state_steps() -> list:
    """(name, lens_new, n_below, ind seed, layer, last, from): a first layer without pruning; a middle layer in which pair 0 stops
    (1 - 3/80 = 0.9625), pair 1 shrinks to 5 tokens on one side and goes on (1 - 10/75 = 0.867) and the stopped pair 2 is handed
    counts that would stop and flag it; a last layer; and the last layer once more without pruning counts, from the same state."""
    i32 = lambda *v: np.array(v, dtype=np.int32)
    return [("first", None, None, 1, 0, False, None),
            ("middle", i32(30, 5, 1, 29, 30, 1), i32(1, 4, 0, 2, 6, 0), 2, 3, False, "first"),
            ("last", i32(9, 4, 2, 9, 20, 2), i32(0, 20, 0, 0, 10, 0), 3, 8, True, "middle"),
            ("last_unpruned", None, None, 4, 8, True, "middle")]


def layer_state_ind(seed: int) -> np.ndarray:
    return perm_rows(7500 + seed, "ls/ind", 2 * LS_B, LS_T).to(torch.int32).numpy() + 1000 * seed


# ---- AdaGML scatter
def scatter_case() -> dict:
    B, T, M = 2, 300, 500
    m0 = torch.floor(W.uniform(7700, "sc/m", (B, T), -60.0, float(T))).long().clamp(min=-1)
    return {"m0": m0.contiguous(), "ms0": W.uniform(7700, "sc/s", (B, T), 0.0, 1.0), "ind0": perm_rows(7700, "sc/i0", B, M)[:, :T].to(torch.int32).contiguous(),
            "ind1": perm_rows(7700, "sc/i1", B, M)[:, :T].to(torch.int32).contiguous(), "m_full": M, "lens0": [300, 17]}


# ---- sampling tail
SAMPLE_C, SAMPLE_HW, SAMPLE_N = (4, 128, 132, 256, 260, 512), (7, 9), 11


def sample_fmap(C: int) -> torch.Tensor:
    """[2, 7, 9, C]: per channel a level of magnitude 0.25 .. 0.5 and either sign plus a pixel term within +-0.05.  The kernel
    forms the source index ((g + 1) / 2) * (size - 1) in float32 — about 1e-6 px away from the float64 index at size 9; with
    neighbouring pixels at most 0.1 apart (0.55 against the zero padding) that is 1e-7 (6e-7) in the sample, and with at least
    four channels of magnitude >= 0.2 the l2-normalised sample moves by no more than a few 1e-7: inside the 2e-6 bar."""
    fh, fw = SAMPLE_HW
    level = W.uniform(8000 + C, "sa/lv", (C,))
    level = torch.where(level >= 0, 0.25 + 0.25 * level, -0.25 + 0.25 * level)
    return (level + 0.05 * W.uniform(8000 + C, "sa/px", (2, fh, fw, C))).contiguous()


def sample_kpts(s: int) -> torch.Tensor:
    """[2, 11, 2].  s = 4: pixel coordinates whose taps all lie on the 7 x 9 map (x in [2, 34], y in [2, 26]).  s = 0: grid
    coordinates, among them -1 and +1 exactly and points up to 0.3 outside, where taps fall on the zero padding."""
    fh, fw = SAMPLE_HW
    if s > 0:
        return torch.stack([W.uniform(8100, "sa/x", (2, SAMPLE_N), 2.0, fw * s - 2.0), W.uniform(8100, "sa/y", (2, SAMPLE_N), 2.0, fh * s - 2.0)], -1).contiguous()
    k = W.uniform(8200, "sa/g", (2, SAMPLE_N, 2))
    edge = torch.tensor([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.05, 0.3], [-1.05, -1.02], [0.2, 1.1], [-1.3, 0.0], [0.5, -1.3]])
    k[0, :8], k[1, 2:10] = edge, edge
    return k.contiguous()


def lookup_case() -> dict:
    H_, W_ = 13, 17
    return {"maps": W.uniform(8300, "lk/m", (2, H_, W_), 0.0, 1.0).contiguous(),
            "kpts": torch.stack([W.uniform(8300, "lk/x", (2, 300), 0.0, float(W_)), W.uniform(8300, "lk/y", (2, 300), 0.0, float(H_))], -1).contiguous(),
            "lens": [300, 3]}


L2_ROWS, L2_COLS = (1, 5), (4, 128, 260)


def l2norm_case(rows: int, cols: int) -> torch.Tensor:
    x = W.uniform(8400 + cols, "l2/x", (rows, cols))
    if rows > 1:
        x[1] = 0.0
    return x.contiguous()


# ---- resize
RESIZE_CASES = (((5, 7), (5, 7)), ((5, 7), (1, 1)), ((5, 7), (11, 3)), ((1, 1), (4, 4)), ((37, 53), (8, 8)))


def resize_case(h: int, w: int) -> torch.Tensor:
    """[3, h, w]: plane + 0.01 y + 0.013 x + 0.002 noise.  The kernel's source coordinate dst * (in - 1) / (out - 1) is float32
    (up to 4e-6 px from the float64 one at 37 -> 8 rows); neighbours at most 0.02 apart keep that below 1e-7 in the value, while a
    tap that is off by a whole pixel is off by 0.01."""
    y, x = torch.arange(h, dtype=torch.float32).view(1, h, 1), torch.arange(w, dtype=torch.float32).view(1, 1, w)
    return (torch.arange(3, dtype=torch.float32).view(3, 1, 1) + 0.01 * y + 0.013 * x + 0.002 * W.uniform(8500 + h, "rs/x", (3, h, w))).contiguous()
