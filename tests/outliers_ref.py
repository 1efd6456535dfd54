"""Statistical outlier removal of a map's points, restated in numpy: the arithmetic csrc/knn.hip performs, in the same order, so
that the device equals this file bit for bit.  It is Open3D's PointCloud::RemoveStatisticalOutliers as include/pram_hip.h states
it (written from knowledge of its source; Open3D is not installed and was never run beside this):

  * d2 = (dx * dx + dy * dy) + dz * dz with dx = x[j] - x[i], in float64;
  * a point's kk = min(k, n) smallest d2, itself included, in ascending order, each square-rooted, added to 0.0 in that order, the
    sum divided by kk;
  * a sum over points cuts them into blocks of BLOCK consecutive indices (PRAM_SOR_BLOCK of include/pram_hip.h, read from there):
    inside a block the terms are added to 0.0 in ascending index, an invalid point (avg not > 0) contributing nothing; the block
    sums are added to 0.0 in ascending block index.  Two passes: the mean, then the squared deviations;
  * threshold = mean + std_ratio * sqrt(sum2 / (nv - 1)); the inliers are the valid points strictly below it; with nv < 2 the
    deviation and the threshold are NaN and nothing is an inlier.

tests/test_outliers_cpu.py compares this file with scipy's k-d tree and numpy's std(ddof=1).
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
_HEADER = (ROOT / "include" / "pram_hip.h").read_text()
BLOCK = int(re.search(r"#define\s+PRAM_SOR_BLOCK\s+(\d+)", _HEADER).group(1))
MAX_K = int(re.search(r"#define\s+PRAM_KNN_MAX_K\s+(\d+)", _HEADER).group(1))
ROWS = 256      # query rows per chunk of the all-pairs table

# the planted scenes the CPU and the GPU tests share: n -> (seed, planted far points)
SCENES = {300: (1, 6), 1500: (2, 30), 4000: (3, 80)}
N_DUP = 4       # copies of a scene's first cluster point: a group of five coincident points, fewer than k = 20, so valid
SURE = 100.0    # a planted point this far from its centre (25 sigma): on the scenes used every one of them has to come out
SIZES = (1, 2, 19, 20, 21, 255, 256, 257, 1023, 1024, 1025, 3000)      # n < k, partial query blocks, partial candidate tiles
KS = (1, 2, 8, 9, 16, 17, 20, 24, 25, 31, 32)      # both sides of every step between two list sizes of the kernel (8, 16, 24, 32)


def scene(n: int, seed: int, n_far: int, n_dup: int = N_DUP, n_clusters: int = 5):
    """A few Gaussian clusters (sigma 4 around centres in +-60 m), ``n_far`` planted points 25 to 300 m from a centre and ``n_dup``
    exact copies of one cluster point, shuffled -> (xyz float64 [n, 3], far_dist float64 [n]: a planted point's distance from its
    centre, 0 for the others, dup bool [n]: the copied point and its copies)."""
    rs = np.random.RandomState(seed)
    n_c = n - n_far - n_dup
    centres = rs.uniform(-60.0, 60.0, size=(n_clusters, 3))
    x = centres[rs.randint(0, n_clusters, size=n_c)] + rs.normal(0.0, 4.0, size=(n_c, 3))
    d = rs.normal(size=(n_far, 3))
    out = rs.uniform(25.0, 300.0, size=n_far)
    far = centres[rs.randint(0, n_clusters, size=n_far)] + d / np.linalg.norm(d, axis=1, keepdims=True) * out[:, None]
    xyz = np.concatenate([x, far, np.repeat(x[:1], n_dup, axis=0)])
    far_dist = np.concatenate([np.zeros(n_c), out, np.zeros(n_dup)])
    dup = (np.arange(n) >= n - n_dup) | ((np.arange(n) == 0) & (n_dup > 0))
    order = rs.permutation(n)
    return np.ascontiguousarray(xyz[order]), far_dist[order], dup[order]


def planted(n: int):
    seed, n_far = SCENES[n]
    return scene(n, seed, n_far)


def sized(n: int) -> np.ndarray:
    """The scene of size n of the sweep over SIZES: no copies below 40 points, a planted point per 50."""
    return scene(n, 100 + n, n // 50, N_DUP if n >= 40 else 0)[0]


PERM_SEED = 17


def case(name: str):
    """A case the GPU tests run -> (xyz, k).  The CPU tests assert the threshold's margin on every one that has a threshold."""
    kind, _, arg = name.partition("_")
    if kind == "n":
        return sized(int(arg)), 20
    if kind == "k":
        return planted(1500)[0], int(arg)
    if kind == "planted":
        return planted(int(arg))[0], 20
    if kind == "lattice":      # 12 x 12 x 12 integers: every k-th distance is tied many times over
        g = np.arange(12, dtype=np.float64)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), 20
    if kind == "dup25":        # 25 coincident points: each has k - 1 duplicates and more, so none is valid
        return scene(1500, 4, 30, n_dup=24)[0], 20
    if kind == "equal":
        return np.full((300, 3), 2.5), 20
    if kind == "offset":
        return planted(1500)[0] + 1e5, 20
    if kind == "perm":
        x = planted(1500)[0]
        return x[np.random.RandomState(PERM_SEED).permutation(len(x))], 20
    if kind == "big":          # 32 query blocks x 8 candidate tiles
        return scene(8192, 7, 100)[0], 20
    raise KeyError(name)


CASES = tuple(f"n_{n}" for n in SIZES) + tuple(f"k_{k}" for k in KS) + ("planted_300", "planted_4000", "lattice", "dup25", "equal", "offset", "perm", "big")
_restated: dict = {}


def restated(name: str) -> dict:
    """statistical_inliers of a case at std_ratio 2, computed once."""
    if name not in _restated:
        xyz, k = case(name)
        _restated[name] = statistical_inliers(xyz, k, 2.0)
    return _restated[name]


def knn_mean_distance(xyz, k: int) -> np.ndarray:
    """float64 [n]: every point's mean distance to its min(k, n) nearest points, itself included."""
    x = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    n = x.shape[0]
    kk = min(int(k), n)
    assert kk >= 1
    avg = np.empty(n, dtype=np.float64)
    for r0 in range(0, n, ROWS):
        q = x[r0:r0 + ROWS]
        dx, dy, dz = (x[None, :, c] - q[:, None, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        small = np.sort(np.partition(d2, kk - 1, axis=1)[:, :kk], axis=1) if kk < n else np.sort(d2, axis=1)
        root = np.sqrt(small)
        s = np.zeros(q.shape[0], dtype=np.float64)
        for c in range(kk):
            s = s + root[:, c]
        avg[r0:r0 + ROWS] = s / float(kk)
    return avg


def blocked_sum(terms: np.ndarray, valid: np.ndarray) -> float:
    """The valid terms, added to 0.0 in ascending index inside every block of BLOCK indices; the block sums in block order."""
    acc = 0.0
    for b0 in range(0, terms.shape[0], BLOCK):
        s = 0.0
        for t, ok in zip(terms[b0:b0 + BLOCK].tolist(), valid[b0:b0 + BLOCK].tolist()):
            if ok:
                s = s + t
        acc = acc + s
    return acc


def select(avg: np.ndarray, std_ratio: float) -> dict:
    avg = np.asarray(avg, dtype=np.float64)
    valid = avg > 0.0
    nv = int(valid.sum())
    with np.errstate(all="ignore"):
        mean = np.float64(blocked_sum(avg, valid)) / np.float64(nv)
        dev = avg - mean
        sum2 = blocked_sum(dev * dev, valid)
        if nv >= 2:
            std = np.sqrt(np.float64(sum2) / np.float64(nv - 1))
            threshold = mean + np.float64(std_ratio) * std
        else:
            std = threshold = np.float64("nan")
        mask = valid & (avg < threshold)
    return {"mask": mask, "inlier_ids": np.nonzero(mask)[0].astype(np.int64), "avg_distance": avg, "mean": float(mean), "std": float(std),
            "threshold": float(threshold), "n_valid": nv}


def statistical_inliers(xyz, nb_neighbors: int = 20, std_ratio: float = 2.0) -> dict:
    if nb_neighbors < 1 or not std_ratio > 0:
        raise ValueError("needs nb_neighbors >= 1 and std_ratio > 0")
    return select(knn_mean_distance(xyz, nb_neighbors), std_ratio)


def margin(r: dict) -> float:
    """min |avg - threshold| / threshold over the valid points: what keeps the mask apart from the last bits of the threshold."""
    v = r["avg_distance"][r["avg_distance"] > 0.0]
    return float(np.abs(v - r["threshold"]).min() / r["threshold"])
