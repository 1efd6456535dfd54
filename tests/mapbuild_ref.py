"""numpy restatement of the two map-building stages of the reference's recognition/recmap.py that pram_amd.localization.mapbuild
runs on the device, and the scene the tests share.

  * assign_point_descriptors: RecMap.assign_point3D_descriptor (recmap.py:124-194), in float64 with an explicitly symmetric Gram
    matrix (upper triangle, mirrored).  The sum over the 128 dimensions is taken in the kernel's order (dot128 below; the
    products of two fp32 values are exact in float64), so the kernel's medians are reproduced bit for bit.
  * select_reference_frames: find_best_vrf_by_covisibility (recmap.py:263-355) and the two `continue`s of the loop around it in
    RecMap.create_virtual_frame_3 (recmap.py:369-403), on store frame indices, with a trace of the branches taken.
"""
from __future__ import annotations

import numpy as np

SEED = 20240207
F, ROWS, FRAME_ID0, UNHELD = 12, 300, 100, 999
SHORT, ROW_LDS = 32, 512      # the kernel's path boundaries (include/pram_hip.h: PRAM_MAPBUILD_SHORT_TRACK, PRAM_MAPBUILD_ROW_LDS)
VRF_PARAMS = dict(min_obs=120, topk_imgs=5, n_vrf=3, min_cover_ratio=0.9, gain_floor=0.01)
IGNORED_FRAME, OUTSIDE_FRAME, ZERO_Z_FRAME = 11, 7, 6
WIDTH, HEIGHT, INTRINSICS = 640, 480, (500.0, 510.0, 320.0, 240.0)


# ------------------------------------------------------------------------------------------------ stage 1
_BUTTERFLY = [np.arange(32) ^ o for o in (16, 8, 4, 2, 1)]


def dot128(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """<a, b> over the last axis (128) of float64 arrays holding fp32 values, in the kernel's order: the products are exact, groups
    of four dimensions are added in ascending order, and the 32 group sums are added by a butterfly (l with l ^ 16, 8, 4, 2, 1)."""
    p = a * b
    p = p.reshape(p.shape[:-1] + (32, 4))
    q = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    for partner in _BUTTERFLY:
        q = q + q[..., partner]
    return q[..., 0]


def gram_batch(A: np.ndarray) -> np.ndarray:
    """A [g, n, 128] float32 -> 2 - 2 A A^T [g, n, n] float64: the upper triangle, mirrored (recmap.py:150-151)."""
    A = A.astype(np.float64)
    g, n, d = A.shape
    acc = np.zeros((g, n, n), dtype=np.float64)
    for i in range(n):
        acc[:, i, :] = dot128(A[:, i:i + 1, :], A)
    up = np.triu(2.0 - 2.0 * acc)
    return up + np.triu(up, 1).transpose(0, 2, 1)


def choose(G: np.ndarray):
    """[g, n, n] -> (np.argmin(np.median(dist, axis=-1)) per matrix, the medians [g, n]) (recmap.py:152-153)."""
    med = np.median(G, axis=-1)
    return np.argmin(med, axis=-1), med


def entry_rows(frame_off, trk_frame, trk_kpt):
    """The store row of every track entry, -1 for a dropped one: an image the map does not hold (recmap.py:140-141), and — where
    the reference would raise — a frame index out of range or a keypoint index outside its frame."""
    n_frames = len(frame_off) - 1
    f = np.asarray(trk_frame, dtype=np.int64)
    k = np.asarray(trk_kpt, dtype=np.int64)
    ok = (f >= 0) & (f < n_frames) & (k >= 0)
    fc = np.clip(f, 0, max(n_frames - 1, 0))
    ok &= k < (frame_off[fc + 1] - frame_off[fc])
    return np.where(ok, frame_off[fc] + k, -1)


def assign_point_descriptors(descriptors, frame_off, trk_off, trk_frame, trk_kpt):
    """-> (choice int32 [P]: the position in the track of the chosen entry, -1 with nothing kept; desc float32 [P, 128]; medians: a
    list of (kept positions, their medians) per point)."""
    rows = entry_rows(np.asarray(frame_off, dtype=np.int64), trk_frame, trk_kpt)
    P = len(trk_off) - 1
    choice = np.full(P, -1, dtype=np.int32)
    desc = np.zeros((P, 128), dtype=np.float32)
    medians = [None] * P
    groups = {}
    for p in range(P):
        e = rows[trk_off[p]:trk_off[p + 1]]
        pos = np.nonzero(e >= 0)[0]
        medians[p] = (pos, np.zeros(0))
        if len(pos):
            groups.setdefault(len(pos), []).append((p, pos, e[pos]))
    for n, items in groups.items():
        A = np.stack([descriptors[r] for _, _, r in items])
        best, med = choose(gram_batch(A))      # n = 1: the reference takes the only row (recmap.py:146-147), and so does this
        for (p, pos, r), b, m in zip(items, best, med):
            choice[p], desc[p], medians[p] = pos[b], descriptors[r[b]], (pos, m)
    return choice, desc, medians


# ------------------------------------------------------------------------------------------------ stage 2
def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def reproject(cam, xyzs):
    """recmap.py:243-261 with the camera row (qvec, tvec, fx, fy, cx, cy, width, height)."""
    Tcw = np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = qvec2rotmat(cam[0:4]), cam[4:7]
    K = np.identity(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = cam[7], cam[8], cam[9], cam[10]
    homo = np.hstack([xyzs, np.ones((xyzs.shape[0], 1))])
    kpts = (K @ ((Tcw @ homo.transpose())[:3, :])).transpose()
    with np.errstate(divide="ignore", invalid="ignore"):
        kpts[:, 0] = kpts[:, 0] / kpts[:, 2]
        kpts[:, 1] = kpts[:, 1] / kpts[:, 2]
    return kpts


def find_best_vrf(p3d_id_list, frame_point_ids, point_frames, ignored, min_obs, topk_imgs, n_vrf, min_cover_ratio, gain_floor, trace):
    """recmap.py:263-355.  frame_point_ids[f]: the ids on frame f's rows; point_frames: point id -> its frames, duplicates kept."""
    all_img_ids, img_ids_full, img_id_obs = [], [], {}
    for pid in p3d_id_list:
        if pid not in point_frames:      # :270
            trace["lacking"] = True
            continue
        for iid in point_frames[pid]:
            if iid in all_img_ids:      # :276
                continue
            if ignored[iid]:      # :279-287
                trace["ignored"] = True
                continue
            n_valid = int((frame_point_ids[iid] > 0).sum())      # :289
            img_ids_full.append(iid)
            if n_valid < min_obs:
                continue
            all_img_ids.append(iid)
            img_id_obs[iid] = n_valid
    top = sorted(img_id_obs.items(), key=lambda item: item[1], reverse=True)      # :299
    trace["count_tie"] = len({c for _, c in top}) < len(top)
    all_img_ids = []
    for item in top:
        all_img_ids.append(item[0])
        if len(all_img_ids) >= topk_imgs:
            trace["topk_cut"] = len(top) > len(all_img_ids)
            break
    if len(all_img_ids) == 0:      # :307-309
        trace["fallback"] = len(img_ids_full) > 0
        all_img_ids = img_ids_full
    p3d_id_array = np.array(p3d_id_list)
    trace["repeated"] = len(set(p3d_id_list)) < len(p3d_id_list)
    img_observations = {}
    for img_id in all_img_ids:      # :313-322
        mask = np.zeros(len(p3d_id_list), dtype=bool)
        for pid in frame_point_ids[img_id][frame_point_ids[img_id] > 0].tolist():
            found = np.where(p3d_id_array == pid)[0]
            if found.shape[0] == 0:
                continue
            mask[found[0]] = True
        img_observations[img_id] = mask
    unobserved = np.ones(len(p3d_id_list), dtype=bool)
    candidates, total = [], 0
    trace["stop"] = "coverage"
    while total < min_cover_ratio:      # :328-353
        best_id, best_obs, n_best = -1, -1, 0
        for im_id in all_img_ids:
            if im_id in candidates:
                continue
            obs_i = int(np.sum(img_observations[im_id] * unobserved))
            if obs_i > best_obs:
                best_id, best_obs, n_best = im_id, obs_i, 1
            elif obs_i == best_obs:
                n_best += 1
        if best_id < 0:
            trace["stop"] = "none left"
            break
        trace["gain_tie"] = trace.get("gain_tie", False) or n_best > 1
        trace["zero_gain"] = trace.get("zero_gain", False) or best_obs == 0
        candidates.append(best_id)
        unobserved[img_observations[best_id]] = False
        total = 1 - np.sum(unobserved) / len(p3d_id_list)
        if best_obs / len(p3d_id_list) < gain_floor:
            trace["stop"] = "gain floor"
            break
        if len(candidates) >= n_vrf:
            trace["stop"] = "n_vrf"
            break
    return candidates


def select_reference_frames(landmarks, frame_point_ids, point_frames, point_xyz, ignored, cams, min_obs, topk_imgs, n_vrf,
                            min_cover_ratio, gain_floor):
    """landmarks: lists of point ids -> (one list of kept store frame indices per landmark, one trace dict per landmark)."""
    out, traces = [], []
    for pts in landmarks:
        pts = [int(p) for p in pts]
        trace = {"id0": 0 in pts, "drop7": False, "drop8": False}
        kept = []
        chosen = find_best_vrf(pts, frame_point_ids, point_frames, ignored, min_obs, topk_imgs, n_vrf, min_cover_ratio, gain_floor,
                               trace) if pts else []
        for img_id in chosen:      # :369-403
            orig = set(p for p in frame_point_ids[img_id].tolist() if p in point_frames and p >= 0)
            orig_xyzs = [point_xyz[p] for p in pts if p in orig]
            if len(orig_xyzs) == 0:
                trace["drop7"] = True
                continue
            k = reproject(cams[img_id], np.array(orig_xyzs))
            inside = (k[:, 0] >= 0) & (k[:, 0] < cams[img_id][11]) & (k[:, 1] >= 0) & (k[:, 1] < cams[img_id][12])
            if not inside.any():
                trace["drop8"] = True
                continue
            kept.append(img_id)
        trace["chosen"] = list(chosen)
        out.append(kept)
        traces.append(trace)
    return out, traces


# ------------------------------------------------------------------------------------------------ the scene
# which landmark of the scene takes which branch (asserted from the traces in tests/test_mapbuild_cpu.py)
LM_COUNT_GAIN_TIES_COVERAGE, LM_FALLBACK_NONE_LEFT, LM_TOPK_CUT_NVRF, LM_ZERO_GAIN_FLOOR = 0, 1, 2, 3
LM_IGNORED_ID0_LACKING_REPEATED, LM_DROP7, LM_DROP8, LM_EMPTY = 4, 5, 6, 7
TARGET_OBS = [200, 200, 200, 200, 180, 170, 160, 150, 40, 40, 40, 250]      # rows with id > 0 per frame


_scene_cache = {}


def scene(seed: int = SEED) -> dict:
    """The shared scene (cached; treat as read-only): F frames of ROWS rows, the tracks of about 2000 points as CSR and as the
    dict build_store_inputs takes, 8 landmarks, and the restatement's results."""
    if seed in _scene_cache:
        return _scene_cache[seed]
    rng = np.random.default_rng(seed)
    n_rows = F * ROWS
    frame_off = np.arange(F + 1, dtype=np.int32) * ROWS
    centres = rng.standard_normal((8, 128))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    d = centres[np.arange(n_rows) % 8] + 0.6 * rng.standard_normal((n_rows, 128))
    descriptors = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    # ---- the landmarks: points 1.. with their table lists (frame indices, in COLMAP's order) and the frames whose rows carry them
    row_ids = [[] for _ in range(F)]      # ids placed on each frame's rows, in row order
    table, where, xyz = {}, {}, {}
    next_id = [1]

    def place(pid, frames):
        for f in frames:
            where.setdefault(pid, {})[f] = len(row_ids[f])
            row_ids[f].append(pid)

    def new_points(n, lists, z=None):
        ids = list(range(next_id[0], next_id[0] + n))
        next_id[0] += n
        for p in ids:
            table[p] = list(lists)
            zz = float(z) if z is not None else float(rng.uniform(5.5, 8.0))
            xyz[p] = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), zz])
        return ids

    landmarks = [None] * 8
    # 0: frames 2, 0, 1 tie in count (order: first encounter) and frames 2 and 0 tie in gain; stops at full coverage
    a = new_points(30, [2, 0, 1])
    for p in a[0:20]:
        place(p, [2])
    for p in a[10:30]:
        place(p, [0])
    for p in a[0:10]:
        place(p, [1])
    landmarks[LM_COUNT_GAIN_TIES_COVERAGE] = a
    # 1: only frames below min_obs (9 then 8, 9 listed twice): the fallback list; 30 % + 30 %, then no candidate is left
    a = new_points(20, [9, 8, 9])
    for p in a[0:6]:
        place(p, [9])
    for p in a[6:12]:
        place(p, [8])
    landmarks[LM_FALLBACK_NONE_LEFT] = a
    # 2: eight frames reach min_obs, cut to five (3, 2, 1, 0 tie and keep their encounter order, then 4); frame 5, which sees every
    # point, is cut away; 15 % per pick, stops at n_vrf
    a = new_points(40, [7, 6, 5, 4, 3, 2, 1, 0])
    for i, f in enumerate([3, 2, 1, 0, 4]):
        for p in a[6 * i:6 * i + 6]:
            place(p, [f])
    for p in a:
        place(p, [5])
    landmarks[LM_TOPK_CUT_NVRF] = a
    # 3: frame 5 sees a subset of frame 4's points: a pick of gain 0, which the gain floor stops at
    a = new_points(20, [4, 5])
    for p in a[0:10]:
        place(p, [4])
    for p in a[0:5]:
        place(p, [5])
    landmarks[LM_ZERO_GAIN_FLOOR] = a
    # 4: id 0, an id the table lacks (7777), a repeated id, and the ignored frame 11, which sees everything and is listed first
    a = new_points(10, [11, 1, 0])
    table[0], xyz[0] = [1], np.array([0.1, -0.2, 6.0])
    pts = [a[0], 0, a[1], 7777, a[1]] + a[2:]
    for p in [a[0], 0, a[1], 7777]:
        place(p, [1])
    for p in [a[1]] + a[2:]:
        place(p, [0])
    for p in [0, 7777] + a:
        place(p, [11])
    landmarks[LM_IGNORED_ID0_LACKING_REPEATED] = pts
    # 5: frame 2 carries only ids of the list that the table lacks: picked (gain 2), then dropped for having no point to project
    a = new_points(10, [2, 3])
    for p in a:
        place(p, [3])
    for p in [8888, 8889]:
        place(p, [2])
    landmarks[LM_DROP7] = a + [8888, 8889]
    # 6: z = 5 exactly; frame 7 looks past every point, frame 6 has them at depth 0: both picked, both dropped; frame 0 stays
    a = new_points(30, [7, 6, 0], z=5.0)
    for p in a[0:15]:
        place(p, [OUTSIDE_FRAME])
    for p in a[15:25]:
        place(p, [ZERO_Z_FRAME])
    for p in a[25:30]:
        place(p, [0])
    landmarks[LM_DROP8] = a
    landmarks[LM_EMPTY] = []

    # ---- rows: the placed ids, fillers (> 0, in no landmark) up to the frame's observation count, an id 0 and -1 beyond
    point3D_ids = np.full(n_rows, -1, dtype=np.int64)
    filler = 50000
    for f in range(F):
        ids = list(row_ids[f])
        n_pos = sum(1 for p in ids if p > 0)
        assert n_pos <= TARGET_OBS[f] and len(ids) <= ROWS - 2
        ids += list(range(filler, filler + TARGET_OBS[f] - n_pos))
        filler += TARGET_OBS[f] - n_pos
        if f not in (1, 11):
            ids.append(0)      # an id 0 on rows of frames where the list of landmark 4 is not concerned
        point3D_ids[f * ROWS:f * ROWS + len(ids)] = ids
        assert int((point3D_ids[f * ROWS:(f + 1) * ROWS] > 0).sum()) == TARGET_OBS[f]

    # ---- cameras: small rotations about the optical centre; frame 7 far to the side, frame 6 five units ahead of the origin
    cams = np.zeros((F, 13))
    for f in range(F):
        q = np.array([1.0, *(0.01 * rng.standard_normal(3))])
        cams[f, 0:4], cams[f, 4:7] = q / np.linalg.norm(q), 0.1 * rng.standard_normal(3)
        cams[f, 7:11], cams[f, 11], cams[f, 12] = INTRINSICS, WIDTH, HEIGHT
    cams[OUTSIDE_FRAME, 0:7] = [1, 0, 0, 0, 100.0, 0, 0]
    cams[ZERO_Z_FRAME, 0:7] = [1, 0, 0, 0, 0, 0, -5.0]
    ignored = np.zeros(F, dtype=np.int32)
    ignored[IGNORED_FRAME] = 1

    # ---- tracks: the landmark points (their table lists; the keypoint is their row where the frame carries them), then about 2000
    # points drawn from the rows of one descriptor cluster each
    tracks, special = [], {}      # tracks: (point id, frame indices, keypoint indices)
    for p in sorted(table):
        tracks.append((p, list(table[p]), [where.get(p, {}).get(f, 0) for f in table[p]]))
    cluster_rows = [np.nonzero(np.arange(n_rows) % 8 == c)[0] for c in range(8)]
    next_id[0] = 2000

    def add_track(rows, name=None, frames=None, kpts=None):
        pid = next_id[0]
        next_id[0] += 1
        fr = [int(r) // ROWS for r in rows] if frames is None else frames
        kp = [int(r) % ROWS for r in rows] if kpts is None else kpts
        tracks.append((pid, fr, kp))
        if name:
            special[name] = pid
        return pid

    def draw(n):
        c = int(rng.integers(8))
        pool = cluster_rows[c] if n <= len(cluster_rows[c]) else np.arange(n_rows)
        return rng.choice(pool, size=n, replace=False)

    for n in [1, 2, 3, 4, 5, 8, 17, 63, 64, 65, 130, 300, SHORT - 1, SHORT, SHORT + 1, ROW_LDS - 1, ROW_LDS, ROW_LDS + 1]:
        add_track(draw(n), name=f"len{n}")
    for n in rng.integers(2, 21, size=1900).tolist():
        add_track(draw(n))
    r = draw(6)
    add_track(r, "dropped_short", frames=[int(r[0]) // ROWS, -1, int(r[2]) // ROWS, int(r[3]) // ROWS, F + 1, int(r[5]) // ROWS],
              kpts=[int(r[0]) % ROWS, 3, int(r[2]) % ROWS, ROWS, 5, -1])
    r = draw(40)
    fr, kp = [int(x) // ROWS for x in r], [int(x) % ROWS for x in r]
    for i in range(0, 40, 4):
        fr[i], kp[i] = ((-1, kp[i]), (fr[i], ROWS + 7), (F, kp[i]), (-7, 0))[(i // 4) % 4]
    add_track(r, "dropped_long", frames=fr, kpts=kp)
    add_track([0, 1, 2, 3], "all_dropped", frames=[-1, F, 0, -1], kpts=[0, 0, ROWS, 5])
    r = draw(3)
    add_track(r, "one_kept", frames=[-1, int(r[1]) // ROWS, -1], kpts=[0, int(r[1]) % ROWS, 0])
    r = draw(7)
    r[4] = r[0]
    add_track(r, "repeat_0_k")
    r = draw(9)
    r[8] = r[3]
    add_track(r, "repeat_k_last")
    add_track(np.repeat(draw(1), 5), "repeat_all")
    r = draw(50)
    r[49] = r[7]
    add_track(r, "repeat_long")

    tracks.sort(key=lambda t: t[0])
    point_ids = np.array([t[0] for t in tracks], dtype=np.int64)
    lens = np.array([len(t[1]) for t in tracks])
    trk_off = np.zeros(len(tracks) + 1, dtype=np.int32)
    trk_off[1:] = np.cumsum(lens)
    trk_frame = np.concatenate([np.asarray(t[1], dtype=np.int32) for t in tracks])
    trk_kpt = np.concatenate([np.asarray(t[2], dtype=np.int32) for t in tracks])
    for p, i in enumerate(point_ids.tolist()):
        if i not in xyz:
            xyz[i] = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(5.5, 8.0)])
    # the same tracks by image id, as COLMAP holds them: an entry outside the store names an image the map does not hold
    image_id = lambda f: FRAME_ID0 + f if 0 <= f < F else UNHELD
    tracks_by_image = {t[0]: (np.array([image_id(f) for f in t[1]], dtype=np.int64), np.array(t[2], dtype=np.int64)) for t in tracks}
    frames = []
    for f in range(F):
        a, b = f * ROWS, (f + 1) * ROWS
        frames.append({"id": FRAME_ID0 + f, "keypoints": np.concatenate([rng.uniform(0, 400, (ROWS, 2)), rng.uniform(0, 1, (ROWS, 1))], 1).astype(np.float32),
                       "descriptors": descriptors[a:b], "xyzs": np.zeros((ROWS, 3)), "point3D_ids": point3D_ids[a:b],
                       "keypoint_segs": np.zeros(ROWS, dtype=np.int32), "width": WIDTH, "height": HEIGHT, "qvec": cams[f, 0:4],
                       "tvec": cams[f, 4:7], "intrinsics": cams[f, 7:11]})

    s = {"frames": frames, "frame_off": frame_off, "descriptors": descriptors, "point3D_ids": point3D_ids, "cams": cams, "ignored": ignored,
         "point_ids": point_ids, "trk_off": trk_off, "trk_frame": trk_frame, "trk_kpt": trk_kpt, "tracks": tracks_by_image,
         "special": special, "landmarks": landmarks, "xyz": xyz, "index_of_point": {p: i for i, p in enumerate(point_ids.tolist())}}
    # ---- the restatement on it
    s["choice"], s["desc"], s["medians"] = assign_point_descriptors(descriptors, frame_off, trk_off, trk_frame, trk_kpt)
    point_frames = {t[0]: [f for f in t[1] if 0 <= f < F] for t in tracks}      # the store's table: unheld images dropped
    frame_point_ids = [point3D_ids[f * ROWS:(f + 1) * ROWS] for f in range(F)]
    s["point_frames"], s["frame_point_ids"] = point_frames, frame_point_ids
    s["vrf"], s["traces"] = select_reference_frames(landmarks, frame_point_ids, point_frames, xyz, ignored, cams, **VRF_PARAMS)
    _scene_cache[seed] = s
    return s
