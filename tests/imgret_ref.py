"""Image retrieval restated in numpy: the arithmetic csrc/imgret.hip performs, in the same order, so that the device equals this
file bit for bit (the similarity search on integer data: exactly; on real vectors it is checked against the float64 product).

  * distance: the sum over d ascending of (double(x_d) - double(c_d))^2, added to 0.0; the lowest centre index wins a tie;
  * residual sums: per (image, centre, d) double(x_d) - double(c_d) over the image's rows with that label, in ascending row index,
    added to 0.0;
  * normalisation: n_c = sqrt(sum over d ascending of v^2), entries v / n_c (a zero block stays zero), g = sqrt of ONE chain over c
    ascending then d ascending of the entries squared, out = float32(entry / g); all zeros for an image without rows;
  * vocabulary: the sampler's picks, then per iteration the residual sums over blocks of BLOCK consecutive rows, the blocks added
    to 0.0 in ascending order, c <- float32(double(c) + sum / count), a centre without a row unchanged;
  * top-k: similarity descending, then index ascending; -1 / 0 padding.

The sums are written as loops over d and over rows: np.sum's pairwise order is not the kernels'.  Below the restatement: the scenes
of tests/test_gpu_imgret.py and tests/test_imgret_cpu.py."""
from __future__ import annotations

import numpy as np

from tests import mapper_ref as MR
from tests import pose_ref as PR
from tests import refine_ref as RR
from tests import triangulation_ref as TR

DIM, MAX_K, MAX_TOPK, BLOCK = 128, 256, 64, 1024
F64 = np.float64


# ---------------------------------------------------------------- the stages
def dist2(x, c) -> np.ndarray:
    """[n, k] float64 squared distances, d ascending."""
    xd, cd = np.asarray(x, dtype=np.float32).astype(F64), np.asarray(c, dtype=np.float32).astype(F64)
    s = np.zeros((xd.shape[0], cd.shape[0]), dtype=F64)
    for d in range(DIM):
        t = xd[:, d, None] - cd[None, :, d]
        s = s + t * t
    return s


def assign(x, c):
    s = dist2(x, c)
    lab = np.argmin(s, axis=1)      # the first minimum: the lowest index
    return lab.astype(np.int32), s[np.arange(len(lab)), lab]


def aggregate(x, labels, c, first, count):
    """-> (sums float64 [n_img, k, 128], n_assigned int32 [n_img, k])."""
    xd, cd = np.asarray(x, dtype=np.float32).astype(F64), np.asarray(c, dtype=np.float32).astype(F64)
    k = cd.shape[0]
    sums, n = np.zeros((len(first), k, DIM), dtype=F64), np.zeros((len(first), k), dtype=np.int32)
    for i, (a, m) in enumerate(zip(first, count)):
        for r in range(int(a), int(a) + int(m)):      # ascending row index
            l = int(labels[r])
            if 0 <= l < k:
                sums[i, l] = sums[i, l] + (xd[r] - cd[l])
                n[i, l] += 1
    return sums, n


def normalize(sums) -> np.ndarray:
    sums = np.asarray(sums, dtype=F64)
    n_img, k, _ = sums.shape
    out = np.zeros((n_img, k * DIM), dtype=np.float32)
    for i in range(n_img):
        v = sums[i]
        s = np.zeros(k, dtype=F64)
        for d in range(DIM):
            s = s + v[:, d] * v[:, d]
        nc = np.sqrt(s)
        e = np.zeros_like(v)
        nz = nc > 0.0
        e[nz] = v[nz] / nc[nz, None]
        g2 = 0.0
        for t in (e * e).ravel().tolist():      # c ascending, then d ascending: one chain
            g2 += t
        g = float(np.sqrt(F64(g2)))
        if g > 0.0:
            out[i] = (e / g).ravel().astype(np.float32)
    return out


def vlad(x, c, first, count) -> np.ndarray:
    labels, _ = assign(x, c)
    return normalize(aggregate(x, labels, c, first, count)[0])


def initial_rows(n: int, k: int, seed: int) -> np.ndarray:
    """The sampler recipe of include/pram_hip.h (pram_pose_hypotheses): key = sm64(sm64(seed)), pick j = mulhi64(sm64(key + j), n - j),
    stepped over the earlier picks in ascending order."""
    U = np.uint64
    key = PR.sm64(PR.sm64(np.array([seed & 0xFFFFFFFFFFFFFFFF], dtype=U)))[0]
    picks, earlier = [], []
    for j in range(k):
        with np.errstate(over="ignore"):
            w = int(PR.sm64(np.array([key], dtype=U) + U(j))[0])
        i = (w * (n - j)) >> 64
        for e in earlier:
            i += i >= e
        picks.append(i)
        earlier = sorted(earlier + [i])
    return np.array(picks, dtype=np.int64)


def lloyd_step(x, c):
    """One iteration -> (new centres float32, counts)."""
    x, c = np.asarray(x, dtype=np.float32), np.asarray(c, dtype=np.float32)
    n = len(x)
    labels, _ = assign(x, c)
    first = np.arange(0, n, BLOCK)
    sums, cnt = aggregate(x, labels, c, first, np.minimum(BLOCK, n - first))
    total, total_n = np.zeros((c.shape[0], DIM), dtype=F64), np.zeros(c.shape[0], dtype=np.int64)
    for b in range(len(first)):      # ascending block order, added to 0.0
        total = total + sums[b]
        total_n = total_n + cnt[b]
    new = c.copy()
    has = total_n > 0
    new[has] = (c[has].astype(F64) + total[has] / total_n[has, None].astype(F64)).astype(np.float32)
    return new, total_n


def train_vocabulary(x, k: int, iters: int = 20, seed: int = 0) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    c = x[initial_rows(len(x), k, seed)].copy()
    for _ in range(iters):
        c, _ = lloyd_step(x, c)
    return c


def topk(S, k: int, exclude=None, db_valid=None):
    """S [nq, nd] similarities (any dtype with exact comparisons) -> (idx int32 [nq, k], sim [nq, k] of S's dtype): similarity
    descending, then index ascending; -1 / 0 beyond the allowed."""
    S = np.asarray(S)
    nq, nd = S.shape
    idx, sim = np.full((nq, k), -1, dtype=np.int32), np.zeros((nq, k), dtype=S.dtype)
    for i in range(nq):
        ok = np.ones(nd, dtype=bool) if db_valid is None else np.asarray(db_valid).astype(bool).copy()
        if exclude is not None and 0 <= int(exclude[i]) < nd:
            ok[int(exclude[i])] = False
        cand = np.nonzero(ok)[0]
        order = cand[np.lexsort((cand, -S[i, cand]))][:k]
        idx[i, :len(order)], sim[i, :len(order)] = order, S[i, order]
    return idx, sim


def unique_pairs(idx) -> list:
    """formats.find_unique_new_pairs' rule on the lists, row-major."""
    seen, pairs = set(), []
    for i, row in enumerate(np.asarray(idx).tolist()):
        for j in row:
            if j >= 0 and (i, j) not in seen and (j, i) not in seen:
                seen.add((i, j))
                pairs.append((i, j))
    return pairs


def flat(frames):
    """Frame dicts -> (rows float32 [n, 128], first, count)."""
    lens = np.array([len(f["descriptors"]) for f in frames], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    return np.concatenate([np.asarray(f["descriptors"], dtype=np.float32).reshape(-1, DIM) for f in frames]), off[:-1], lens


def topk_eps(L: int) -> float:
    """The bound of an fp32 fmaf chain of length L on unit vectors against the float64 product: 2 L 2^-24 (L u / (1 - L u) times
    sum |a_i b_i| <= |a| |b|, about 1; the 2 covers the denominator and the rounding of the norms)."""
    return 2.0 * L * 2.0 ** -24


# ---------------------------------------------------------------- the planted covisible scene (refine_ref.covisible_scene)
# The seed of the vocabulary is chosen here, on the restatement: frame 5 shares 110 points with frame 4 (155 rows) and 93 with frame
# 6 (113 rows), which a cosine similarity sees as 110 / sqrt(138 * 155) = 0.752 against 93 / sqrt(138 * 113) = 0.745, so which of the
# two comes first depends on the vocabulary.  Of the seeds 0 .. 23 only 12, 20 and 21 put frame 4 first; 12 does with a gap of 0.027
# (tests/test_imgret_cpu.py holds every margin of the scene against the arithmetic's bound).
COVIS_K, COVIS_ITERS, COVIS_SEED = 16, 20, 12
COVIS_QUERY_TOP2 = ((0, 1), (3, 4), (6, 7))      # the two frames that share most pool points with the windows of queries 0 to 2
_cache: dict = {}


def shared_ids(a, b) -> int:
    a, b = np.asarray(a), np.asarray(b)
    return len(np.intersect1d(a[a >= 0], b[b >= 0]))


def covisible():
    """-> dict: the map, the queries, the planted cameras, per frame pair the shared point ids, per (query, frame) the shared pool
    points, and the restatement's vocabulary and vectors of frames and queries."""
    if "covis" in _cache:
        return _cache["covis"]
    m, qs, planted = RR.covisible_scene()
    frames = m["frames"]
    F = len(frames)
    share = np.array([[shared_ids(frames[a]["point3D_ids"], frames[b]["point3D_ids"]) if a != b else -1 for b in range(F)] for a in range(F)])
    pool_of = [np.arange(RR.FRAME_STEP * f, RR.FRAME_STEP * f + RR.FRAME_ROWS[f] - (RR.LOST_ROWS if f == 1 else 0)) for f in range(F)]
    q_share = np.array([[len(np.intersect1d(q["pool"][q["pool"] >= 0], pool_of[f])) for f in range(F)] for q in qs])
    x, first, count = flat(frames)
    c = train_vocabulary(x, COVIS_K, COVIS_ITERS, COVIS_SEED)
    v_frames = vlad(x, c, first, count)
    qx, qfirst, qcount = flat([{"descriptors": q["descriptors"]} for q in qs])
    v_queries = vlad(qx, c, qfirst, qcount) if len(qx) else np.zeros((len(qs), COVIS_K * DIM), dtype=np.float32)
    _cache["covis"] = dict(map=m, queries=qs, planted=planted, share=share, q_share=q_share, centres=c, v_frames=v_frames, v_queries=v_queries,
                           rows=x, first=first, count=count)
    return _cache["covis"]


# ---------------------------------------------------------------- the planted street scene
STREET_FRAMES, STREET_STEP, STREET_DEPTH, STREET_POINTS = 16, 2.0, 8.0, 2400
STREET_LENGTH = 40.0                  # about four fields of view at STREET_DEPTH (64 degrees: 10 units)
STREET_K, STREET_ITERS, STREET_SEED, STREET_MATCHED, STREET_GAP = 16, 20, 0, 4, 3
STREET_MIN_SHARE = 100                # planted points every listed pair must share: the restatement's fewest is 110 (frames 0 and 4)
WRONG_SHARE, NOISE_PX = MR.WRONG_SHARE, MR.NOISE_PX


def street_scene(seed: int = 31) -> dict:
    """16 frames over the five camera models in turn move along a line and look sideways at a slab of points about four fields of
    view long: a frame shares points only with its neighbours (about four fifths with the next, nothing from five on).  Keypoints
    by mapper_ref.planted_scene's recipe (0.5 px of noise, a detection of nothing now and then); ``where``: (frame, point) -> keypoint;
    ``neighbour_pairs``: frames at most STREET_GAP apart."""
    if ("street", seed) in _cache:
        return _cache[("street", seed)]
    rng = np.random.RandomState(seed)
    F = STREET_FRAMES
    cx = 5.0 + STREET_STEP * np.arange(F)
    centres = [np.array([x, 0.2 * np.sin(0.7 * f), 0.0]) for f, x in enumerate(cx)]
    targets = [c + np.array([0.0, 0.0, 1.0]) for c in centres]
    s = TR._base([TR.CAMERAS[f % 5] for f in range(F)], centres, targets)
    xyz = rng.uniform([0.0, -2.5, STREET_DEPTH - 2.0], [STREET_LENGTH, 2.5, STREET_DEPTH + 2.0], size=(STREET_POINTS, 3))
    kps, where = [[] for _ in range(F)], {}
    for f in range(F):
        px, z = TR.project(s, f, xyz)
        # far off the axis the radial models fold a point back into the image: only what the lens really sees counts
        front = np.abs(xyz[:, 0] - centres[f][0]) < 0.75 * z
        for pt in rng.permutation(len(xyz)).tolist():
            if front[pt] and z[pt] > 0.5 and 8.0 <= px[pt, 0] < TR.WIDTH - 8.0 and 8.0 <= px[pt, 1] < TR.HEIGHT - 8.0:
                kps[f].append(tuple(px[pt] - 0.5 + rng.normal(0.0, NOISE_PX, size=2)))
                where[(f, pt)] = len(kps[f]) - 1
                if rng.uniform() < 0.25:
                    kps[f].append(tuple(rng.uniform([8.0, 8.0], [TR.WIDTH - 8.0, TR.HEIGHT - 8.0])))      # a detection of nothing
    s.update(pairs=np.zeros((0, 2), dtype=np.int64), matches=[], xyz=xyz, where=where)
    s = TR._finish(s, kps)
    seen = [set(pt for (g, pt) in where if g == f) for f in range(F)]
    s["share"] = np.array([[len(seen[a] & seen[b]) if a != b else -1 for b in range(F)] for a in range(F)])
    s["neighbour_pairs"] = [(a, b) for a in range(F) for b in range(a + 1, min(a + STREET_GAP + 1, F))]
    _cache[("street", seed)] = s
    return s


def street_features(s: dict, noise: float = 0.25, seed: int = 32) -> list:
    """Descriptors by mapper_ref.planted_features' recipe: a unit descriptor per planted point, every keypoint of that point the
    descriptor plus noise, a keypoint of nothing a descriptor of its own -> the feature frames."""
    rng = np.random.RandomState(seed)
    unit = lambda x: (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)
    desc = unit(rng.standard_normal((len(s["xyz"]), DIM)))
    fo, frames = s["frame_off"], []
    for f in range(s["n_frames"]):
        n = int(fo[f + 1] - fo[f])
        d = unit(rng.standard_normal((n, DIM)))
        own = [(k, pt) for (g, pt), k in s["where"].items() if g == f]
        k, pt = np.array(own).T
        d[k] = unit(desc[pt] + noise / np.sqrt(float(DIM)) * rng.standard_normal((len(pt), DIM)))
        kp = np.concatenate([s["keypoints"][fo[f]:fo[f + 1]], rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1)
        frames.append({"keypoints": kp, "descriptors": d, "width": TR.WIDTH, "height": TR.HEIGHT})
    return frames


def street_matches(s: dict, pairs, seed: int = 33) -> list:
    """The matches of the requested pairs from the shared points (nine in ten of them), a fifth of every list wrong: between
    keypoints no right match uses.  Per pair int64 [m, 2] in the pair's own orientation; the list of a pair does not depend on the
    other pairs requested."""
    where, fo, out = s["where"], s["frame_off"], []
    n_pts = len(s["xyz"])
    for a, b in pairs:
        a, b = int(a), int(b)
        lo, hi = min(a, b), max(a, b)
        rng = np.random.RandomState(seed + 1000 * lo + hi)
        good = [(where[(lo, pt)], where[(hi, pt)]) for pt in range(n_pts) if (lo, pt) in where and (hi, pt) in where and rng.uniform() < 0.9]
        used0, used1 = {x[0] for x in good}, {x[1] for x in good}
        free0 = [i for i in rng.permutation(int(fo[lo + 1] - fo[lo])).tolist() if i not in used0]
        free1 = [j for j in rng.permutation(int(fo[hi + 1] - fo[hi])).tolist() if j not in used1]
        n_wrong = min(int(round(len(good) * WRONG_SHARE / (1.0 - WRONG_SHARE))), len(free0), len(free1))
        m = good + list(zip(free0[:n_wrong], free1[:n_wrong]))
        m = np.array([m[i] for i in rng.permutation(len(m)).tolist()], dtype=np.int64).reshape(-1, 2)
        out.append(m if a == lo else m[:, ::-1].copy())
    return out


def street():
    """The scene, its features, and the restatement's vocabulary, vectors, lists and pairs."""
    if "street_all" in _cache:
        return _cache["street_all"]
    s = street_scene()
    frames = street_features(s)
    x, first, count = flat(frames)
    c = train_vocabulary(x, STREET_K, STREET_ITERS, STREET_SEED)
    v = vlad(x, c, first, count)
    S = v.astype(F64) @ v.astype(F64).T
    idx, sim = topk(S, STREET_MATCHED, exclude=np.arange(len(v)))
    _cache["street_all"] = dict(scene=s, frames=frames, centres=c, vectors=v, S=S, idx=idx, sim=sim, pairs=unique_pairs(idx))
    return _cache["street_all"]


# ---------------------------------------------------------------- the cases of the kernel tests (shared by the CPU and the GPU file)
ASSIGN_ROWS, ASSIGN_K = (1, 63, 64, 65, 257, 1025), (1, 2, 16, 64, 256)


def assign_case(n: int, k: int):
    """Rows scattered about k centres, with duplicate centres planted (the last is the first; from 16 on centre 7 is centre 3), so
    that every row near one of them meets an exact tie."""
    rng = np.random.RandomState(1000 * k + n)
    c = rng.standard_normal((k, DIM)).astype(np.float32)
    if k >= 2:
        c[k - 1] = c[0]
    if k >= 16:
        c[7] = c[3]
    x = (c[rng.randint(0, k, size=n)] + 0.3 * rng.standard_normal((n, DIM))).astype(np.float32)
    return x, c


FLAT_COUNTS = (0, 1, 65, 300)                      # an image without rows, one of one row (15 centres nobody chooses), two longer
PADDED_N, PADDED_COUNTS = 80, (0, 37, 79)          # the padded layout: counts < N, NaN behind every count
AGG_K = 16


def aggregate_case():
    """-> (centres, the flat layout (rows, first, count), the padded batch [B, N, 128] with NaN behind every count, its counts)."""
    rng = np.random.RandomState(77)
    c = rng.standard_normal((AGG_K, DIM)).astype(np.float32)
    near = lambda n: (c[rng.randint(0, AGG_K, size=n)] + 0.5 * rng.standard_normal((n, DIM))).astype(np.float32)
    cnt = np.array(FLAT_COUNTS, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    x = near(int(cnt.sum()))
    batch = np.full((len(PADDED_COUNTS), PADDED_N, DIM), np.nan, dtype=np.float32)
    for b, m in enumerate(PADDED_COUNTS):
        batch[b, :m] = near(m)
    return c, (x, first, cnt), batch, np.array(PADDED_COUNTS, dtype=np.int64)


def padded_vlad(batch, counts, c):
    """The restatement on the padded layout: only the rows below a count exist."""
    rows = np.concatenate([batch[b, :m] for b, m in enumerate(counts)] + [np.zeros((0, DIM), dtype=np.float32)])
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    labels, _ = assign(rows, c) if len(rows) else (np.zeros(0, dtype=np.int32), None)
    sums, n = aggregate(rows, labels, c, first, counts)
    return sums, n, normalize(sums)


VOCAB_N, VOCAB_K, VOCAB_ITERS, VOCAB_SEED, VOCAB_STARVED, VOCAB_TWIN = 1025, 16, 3, 5, 9, 4


def vocab_case():
    """1025 rows (one past a block) about 16 clusters; the row the sampler picks for centre VOCAB_STARVED is made a copy of the row
    it picks for centre VOCAB_TWIN, so the two start equal, every tie goes to the lower index and VOCAB_STARVED gets no row in the
    first iteration."""
    rng = np.random.RandomState(99)
    m = 2.0 * rng.standard_normal((VOCAB_K, DIM))
    x = (m[rng.randint(0, VOCAB_K, size=VOCAB_N)] + rng.standard_normal((VOCAB_N, DIM))).astype(np.float32)
    picks = initial_rows(VOCAB_N, VOCAB_K, VOCAB_SEED)
    x[picks[VOCAB_STARVED]] = x[picks[VOCAB_TWIN]]
    return x, picks


# (nq, nd, L, k): every nq x nd at one length, the lengths, the list sizes (k > nd: the -1 padding)
TOPK_CASES = tuple((nq, nd, 1024, 20) for nq in (1, 33, 65) for nd in (1, 63, 64, 65, 257, 1000)) + \
    tuple((nq, nd, L, 20) for L in (128, 8192) for nq, nd in ((33, 257), (65, 1000))) + \
    tuple((nq, nd, 128, k) for k in (1, 64) for nq, nd in ((33, 63), (65, 1000), (1, 65)))
TOPK_SPLITS = (1, 3, 8)


def topk_int_case(nq: int, nd: int, L: int):
    """Entries from {-1, 0, 1}: every partial sum is an integer below 2^24, so the fp32 chain is exact in any order, and the data is
    full of ties."""
    rng = np.random.RandomState(nq * 7919 + nd * 31 + L)
    q = rng.randint(-1, 2, size=(nq, L)).astype(np.float32)
    db = rng.randint(-1, 2, size=(nd, L)).astype(np.float32)
    if nd > 3:
        db[nd - 1] = db[1]      # a certain tie for every query
    return q, db


def self_exclude(nq: int, nd: int) -> np.ndarray:
    e = np.arange(nq, dtype=np.int32)
    e[e >= nd] = -1
    return e
