// Map building: the two deterministic, data-parallel parts of the reference's landmark generation (recognition/recmap.py).
//   * RecMap.assign_point3D_descriptor (recmap.py:124-194): per 3D point the descriptor of its track with the smallest median
//     distance to the others.  One workgroup per point; a track of at most PRAM_MAPBUILD_SHORT_TRACK entries keeps its rows, its
//     Gram matrix and the rank selection in LDS, a longer one goes row by row through the caller's workspace.
//   * find_best_vrf_by_covisibility and the filter around it in RecMap.create_virtual_frame_3 (recmap.py:263-355, 369-403): the
//     virtual reference frames of every landmark.  One workgroup per landmark; the first-encounter keys, the candidate order, the
//     masks and all greedy rounds in one launch, everything that outgrows LDS in the caller's workspace.
// Float64 throughout where the reference has floating point; integer atomics only (min / or / add, whose results do not depend on
// the order they arrive in); every index read from a table is checked against the size given beside it before it is used.
#include "glue.h"

namespace {

constexpr int MB_SHORT = PRAM_MAPBUILD_SHORT_TRACK;
constexpr int MB_ROW_LDS = PRAM_MAPBUILD_ROW_LDS;
constexpr int MB_ROW4 = 32;      // float4 per staged row
constexpr int MB_MAX_VRF = PRAM_MAPBUILD_MAX_VRF;
constexpr int MB_IDX_LDS = MB_SHORT * MB_ROW4 * 4;      // row indices of a long track that fit the short path's staged rows
constexpr int MB_UNROLL = 8;
static_assert(MB_SHORT == 32, "the short path's argmin is one half wave");
static_assert(MB_ROW_LDS <= MB_SHORT * (MB_SHORT + 1), "the long path's Gram row aliases the short path's matrix");

// <a, b> over the 128 dimensions in float64, by one half wave (32 lanes; lane l holds dimensions 4l .. 4l + 3 of both rows, so a row
// is read with one 16-byte load per lane, 512 contiguous bytes per half wave).  The products of two floats are exact in float64;
// a lane adds its four in ascending order, then a butterfly over the 32 lanes adds the partial sums (lane l with lane l ^ 16,
// then ^ 8, 4, 2, 1: both partners add the same two numbers, so every lane ends with the same sum).  One fixed order for every
// pair: a function of the two rows' values only, and symmetric bit for bit.  The lanes of a half wave call it together.
__device__ __forceinline__ double dot128_half(const float4 x, const float4 y) {
    double q = (double)x.x * (double)y.x;
    q = fma((double)x.y, (double)y.y, q);
    q = fma((double)x.z, (double)y.z, q);
    q = fma((double)x.w, (double)y.w, q);
    return half_wave_sum_f64(q);
}

// numpy's median of the n values that are not NaN among d[0 .. len) by rank counting, into v[0] (the k0-th smallest) and v[1]
// (the k1-th): a value is the k-th smallest when fewer than k + 1 are smaller and at least k + 1 are smaller or equal; equal
// values write the same number.  Every thread of the workgroup calls it; the caller puts a barrier before reading v.
__device__ __forceinline__ void rank_medians(const double* d, int len, int k0, int k1, double* v) {
    for (int j = threadIdx.x; j < len; j += 256) {
        const double x = d[j];
        if (!(x == x)) continue;
        int less = 0, eq = 0;
        for (int t = 0; t < len; ++t) { const double dt = d[t]; less += dt < x; eq += dt == x; }
        if (less <= k0 && k0 < less + eq) v[0] = x;
        if (less <= k1 && k1 < less + eq) v[1] = x;
    }
}

// the store row of track entry (frame f, keypoint k), or -1 for an entry that is dropped
__device__ __forceinline__ int track_row(const int* __restrict__ frame_off, int n_frames, int n_rows, int f, int k) {
    if (f < 0 || f >= n_frames || k < 0) return -1;
    const int r0 = frame_off[f], r1 = frame_off[f + 1];
    if (r0 < 0 || r1 > n_rows || k >= r1 - r0) return -1;
    return r0 + k;
}

__global__ __launch_bounds__(256) void mapbuild_desc_kernel(const float4* __restrict__ desc, const int* __restrict__ frame_off, int n_frames,
                                                            int n_rows, const int* __restrict__ trk_off, const int* __restrict__ trk_frame,
                                                            const int* __restrict__ trk_kpt, int n_entries, long long ws_end, double* ws_d, int* ws_row,
                                                            float4* __restrict__ pt_desc, int* __restrict__ pt_choice) {
    __shared__ float4 s_rows[MB_SHORT * MB_ROW4];
    __shared__ double s_gram[MB_SHORT * (MB_SHORT + 1)];
    __shared__ double s_v[2 * MB_SHORT];
    __shared__ int s_krow[MB_SHORT], s_kpos[MB_SHORT];
    __shared__ int s_n;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    int e0 = trk_off[p], len = trk_off[p + 1] - e0;
    if (e0 < 0 || len < 0 || len > n_entries - e0) len = 0;      // the entry checked the host copy: never taken
    if (len > MB_SHORT && (long long)e0 + len > ws_end) len = 0;      // nor this: the workspace covers every long track
    int choice = -1, row = -1;      // uniform over the workgroup from here on

    if (len <= MB_SHORT) {
        // ---- short track: the kept entries in track order, their rows and the whole Gram matrix in LDS
        if (tid < 64) {
            const int r = tid < len ? track_row(frame_off, n_frames, n_rows, trk_frame[e0 + tid], trk_kpt[e0 + tid]) : -1;
            const unsigned long long bal = __ballot(r >= 0);
            if (r >= 0) {
                const int c = __popcll(bal & ((1ull << lane) - 1ull));
                s_krow[c] = r;
                s_kpos[c] = tid;
            }
            if (tid == 0) s_n = __popcll(bal);
        }
        __syncthreads();
        const int n = s_n;
        if (n > 0) {
            for (int idx = tid; idx < n * 32; idx += 256) {
                const int r = idx >> 5, q = idx & 31;
                s_rows[r * MB_ROW4 + q] = desc[(size_t)s_krow[r] * 32 + q];
            }
            __syncthreads();
            // the upper triangle, mirrored: one half wave per pair
            for (int idx = tid >> 5; idx < n * n; idx += 8) {
                const int i = idx / n, j = idx - i * n;
                if (j < i) continue;      // uniform over the half wave
                const double d = 2.0 - 2.0 * dot128_half(s_rows[i * MB_ROW4 + (tid & 31)], s_rows[j * MB_ROW4 + (tid & 31)]);
                if ((tid & 31) == 0) {
                    s_gram[i * (MB_SHORT + 1) + j] = d;
                    s_gram[j * (MB_SHORT + 1) + i] = d;
                }
            }
            __syncthreads();
            // numpy's median of every row by rank counting: element (i, j) is the k-th smallest of row i when fewer than k + 1
            // are smaller and at least k + 1 are smaller or equal; equal elements write the same value
            const int k0 = (n - 1) >> 1, k1 = n >> 1;
            for (int idx = tid; idx < n * n; idx += 256) {
                const int i = idx / n, j = idx - i * n;
                const double* g = s_gram + i * (MB_SHORT + 1);
                const double v = g[j];
                int less = 0, eq = 0;
                for (int x = 0; x < n; ++x) { less += g[x] < v; eq += g[x] == v; }
                if (less <= k0 && k0 < less + eq) s_v[i] = v;
                if (less <= k1 && k1 < less + eq) s_v[MB_SHORT + i] = v;
            }
            __syncthreads();
            // the first row with the smallest median
            double m = tid < n ? (s_v[tid & (MB_SHORT - 1)] + s_v[MB_SHORT + (tid & (MB_SHORT - 1))]) * 0.5 : __longlong_as_double(0x7ff0000000000000LL);
            int bi = tid < n ? tid : 0x7fffffff;
            if (tid < 64) {
                wave_argmin_f64(m, bi);
                if (tid == 0) s_n = bi < n ? bi : 0;      // a track of NaN rows: in range, no more is promised
            }
            __syncthreads();
            const int best = s_n;
            choice = s_kpos[best];
            row = s_krow[best];
        }
    } else {
        // ---- long track: the rows stay in global memory; row i of the Gram matrix at a time (LDS up to MB_ROW_LDS entries, the
        // workspace beyond), dropped entries as NaN, which no comparison counts
        if (tid == 0) s_n = 0;
        __syncthreads();
        // the store row of every entry, -1 for a dropped one: LDS (the short path's staged rows) up to MB_IDX_LDS entries
        int* rows = len <= MB_IDX_LDS ? reinterpret_cast<int*>(s_rows) : ws_row + e0;
        int cnt = 0;
        for (int j = tid; j < len; j += 256) {
            const int r = track_row(frame_off, n_frames, n_rows, trk_frame[e0 + j], trk_kpt[e0 + j]);
            rows[j] = r;
            cnt += r >= 0;
        }
        cnt = wave_sum_i32(cnt);
        if (lane == 0 && cnt) atomicAdd(&s_n, cnt);
        __syncthreads();
        const int n = s_n;
        const int k0 = (n - 1) >> 1, k1 = n >> 1;
        const bool in_lds = len <= MB_ROW_LDS;      // the Gram row: LDS (the short path's matrix), or the workspace
        double* drow = in_lds ? s_gram : ws_d + e0;
        double best_m = 0.0;
        for (int i = 0; i < len && n > 0; ++i) {
            const int ri = rows[i];      // uniform
            if (ri < 0) continue;
            const float4 a = desc[(size_t)ri * 32 + (tid & 31)];
            // one half wave per row j, 512 contiguous bytes; MB_UNROLL rows requested before the first is used, since a track
            // this long is one workgroup's chain of memory round trips
            for (int j0 = (tid >> 5) * MB_UNROLL; j0 < len; j0 += 8 * MB_UNROLL) {
                int rj[MB_UNROLL];
                float4 y[MB_UNROLL];
#pragma unroll
                for (int u = 0; u < MB_UNROLL; ++u) rj[u] = j0 + u < len ? rows[j0 + u] : -1;
#pragma unroll
                for (int u = 0; u < MB_UNROLL; ++u) y[u] = desc[(size_t)(rj[u] >= 0 ? rj[u] : ri) * 32 + (tid & 31)];
#pragma unroll
                for (int u = 0; u < MB_UNROLL; ++u) {
                    const double d = dot128_half(a, y[u]);
                    if ((tid & 31) == 0 && j0 + u < len) drow[j0 + u] = rj[u] >= 0 ? 2.0 - 2.0 * d : __longlong_as_double(0x7ff8000000000000LL);
                }
            }
            __syncthreads();
            if (in_lds) rank_medians(s_gram, len, k0, k1, s_v);
            else rank_medians(ws_d + e0, len, k0, k1, s_v);
            __syncthreads();
            const double m = (s_v[0] + s_v[1]) * 0.5;
            if (choice < 0 || m < best_m) { best_m = m; choice = i; row = ri; }      // ascending i: a tie keeps the lower position
        }
    }
    if (tid < 32) pt_desc[(size_t)p * 32 + tid] = row >= 0 ? desc[(size_t)row * 32 + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid == 0) pt_choice[p] = choice;
}

// ------------------------------------------------------------------------------------------------ virtual reference frames
template <typename T>
__device__ __forceinline__ T ld_agent(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// what the atomics of a landmark's workgroup wrote is read past this compute unit's vector cache (ld_agent): a line of it may sit
// there from a neighbouring landmark's reads
struct VrfWs { unsigned long long* enc; unsigned long long* ekey; unsigned long long* hkey; int* cand; int* efr; int* hpos; unsigned* mask; unsigned* unobs; int* fcount; };

__device__ __forceinline__ unsigned hash_id(long long id) { return (unsigned)(((unsigned long long)id * 0x9E3779B97F4A7C15ull) >> 32); }

// the first position of id (> 0) in the landmark's list, -1 when the list does not hold it; the table has h > keys slots
__device__ __forceinline__ int vrf_lookup(const unsigned long long* hkey, const int* hpos, unsigned h, long long id) {
    unsigned s = hash_id(id) % h;
    for (unsigned it = 0; it < h; ++it) {
        const unsigned long long k = ld_agent(hkey + s);
        if (k == (unsigned long long)id) return ld_agent(hpos + s);
        if (k == 0ull) return -1;
        s = s + 1 == h ? 0 : s + 1;
    }
    return -1;
}

// recmap.py:289: a frame's observation count = its rows with id > 0.  One workgroup per frame.
__global__ __launch_bounds__(256) void mapbuild_frame_obs_kernel(const long long* __restrict__ ids, const int* __restrict__ frame_off,
                                                                 int n_rows, int* __restrict__ fcount) {
    __shared__ int s4[4];
    const int f = blockIdx.x;
    int r0, r1, c = 0;
    clamped_range(frame_off[f], frame_off[f + 1], n_rows, r0, r1);
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) c += ids[r] > 0;
    c = block_sum_i32<4>(c, s4);
    if (threadIdx.x == 0) fcount[f] = c;
}

__global__ __launch_bounds__(256) void mapbuild_vrf_kernel(const long long* __restrict__ ids, const int* __restrict__ frame_off, int n_frames,
                                                           int n_rows, const long long* __restrict__ pt_ids, const int* __restrict__ pt_off,
                                                           const int* __restrict__ pt_frames, int n_points, int n_entries,
                                                           const double* __restrict__ pt_xyz, const int* __restrict__ lm_off,
                                                           const long long* __restrict__ lm_points, int n_lm_points,
                                                           const int* __restrict__ frame_ignored, const double* __restrict__ frame_cams,
                                                           int min_obs, int topk, int n_vrf, double min_cover, double gain_floor, VrfWs ws,
                                                           int* __restrict__ lm_vrf, int* __restrict__ lm_vrf_n) {
    __shared__ unsigned long long s_u64[4];
    __shared__ int s_i4[4];
    __shared__ int s_chosen[MB_MAX_VRF];
    __shared__ int s_has_zero, s_has_big, s_n_elig, s_flag;
    const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* out = lm_vrf + (size_t)l * n_vrf;
    int o = lm_off[l], n = lm_off[l + 1] - o;
    if (o < 0 || n < 0 || n > n_lm_points - o) n = 0;      // the entry checked the host copy: never taken
    if (n == 0) {
        for (int k = tid; k < n_vrf; k += 256) out[k] = -1;
        if (tid == 0) lm_vrf_n[l] = 0;
        return;
    }
    const int F = n_frames;
    const long long* pts = lm_points + o;
    unsigned long long* enc = ws.enc + (size_t)l * F;
    unsigned long long* ekey = ws.ekey + (size_t)l * F;
    int* cand = ws.cand + (size_t)l * F;
    int* efr = ws.efr + (size_t)l * F;
    const unsigned h = 2u * (unsigned)n + 1u;
    unsigned long long* hkey = ws.hkey + 2 * (size_t)o + l;
    int* hpos = ws.hpos + 2 * (size_t)o + l;
    const int words = (n + 31) >> 5;
    const size_t woff = (size_t)(o >> 5) + l;      // words of the landmarks before this one: at most (o >> 5) + l
    unsigned* mask = ws.mask + woff * F;
    unsigned* unobs = ws.unobs + woff;
    if (tid == 0) { s_has_zero = 0; s_has_big = 0; s_n_elig = 0; }
    __syncthreads();

    // ---- the list's ids > 0 -> first position (hash, integer min), and the first encounter of every frame in the double loop
    // over the list and each point's frame list (recmap.py:269-295): min of (position in the list, position in the frame list)
    for (int q = tid; q < n; q += 256) {
        const long long id = pts[q];
        if (id == 0) s_has_zero = 1;
        if (id > 0) {
            unsigned s = hash_id(id) % h;
            for (unsigned it = 0; it < h; ++it) {
                const unsigned long long prev = atomicCAS(hkey + s, 0ull, (unsigned long long)id);
                if (prev == 0ull || prev == (unsigned long long)id) { atomicMin(hpos + s, q); break; }
                s = s + 1 == h ? 0 : s + 1;
            }
        }
        const int lo = lower_bound_i64(pt_ids, n_points, id);
        if (lo >= n_points || pt_ids[lo] != id) continue;
        int e0, e1;
        clamped_range(pt_off[lo], pt_off[lo + 1], n_entries, e0, e1);
        for (int e = e0; e < e1; ++e) {
            const int f = pt_frames[e];
            if (f >= 0 && f < F && frame_ignored[f] == 0) atomicMin(enc + f, ((unsigned long long)(unsigned)q << 32) | (unsigned)(e - e0));
        }
    }
    __threadfence();
    __syncthreads();

    // ---- candidates: with a frame of min_obs observations those, by count descending then first encounter, cut at topk;
    // without one every encountered frame by first encounter (recmap.py:299-309)
    for (int f = tid; f < F; f += 256)
        if (ld_agent(enc + f) != ~0ull && ws.fcount[f] >= min_obs) s_has_big = 1;
    __syncthreads();
    const bool big = s_has_big != 0;
    const int limit = big ? topk : F;
    for (int f = tid; f < F; f += 256) {
        const unsigned long long ef = ld_agent(enc + f);
        if (ef == ~0ull || (big && ws.fcount[f] < min_obs)) continue;
        const int c = atomicAdd(&s_n_elig, 1);      // an arbitrary slot: the ranks below do not depend on it
        ekey[c] = ef;
        efr[c] = f;
    }
    __syncthreads();
    const int n_elig = s_n_elig;
    for (int c = tid; c < n_elig; c += 256) {
        const unsigned long long kf = ekey[c];
        const int f = efr[c], cf = ws.fcount[f];
        int rank = 0;
        for (int g = 0; g < n_elig; ++g) {
            const unsigned long long kg = ekey[g];
            const int cg = ws.fcount[efr[g]];
            rank += big ? (cg > cf || (cg == cf && kg < kf)) : (kg < kf);
        }
        if (rank < limit) cand[rank] = f;
    }
    __syncthreads();
    const int n_cand = n_elig < limit ? n_elig : limit;

    // ---- masks (recmap.py:311-322): one wave per candidate, a bit per list position whose id a row of the frame carries
    for (int c = wave; c < n_cand; c += 4) {
        const int f = cand[c];
        int r0, r1;
        clamped_range(frame_off[f], frame_off[f + 1], n_rows, r0, r1);
        for (int r = r0 + lane; r < r1; r += 64) {
            const long long id = ids[r];
            if (id <= 0) continue;
            const int pos = vrf_lookup(hkey, hpos, h, id);
            if (pos >= 0 && pos < n) atomicOr(mask + (size_t)c * words + (pos >> 5), 1u << (pos & 31));
        }
    }
    for (int w = tid; w < words; w += 256) unobs[w] = (w == words - 1 && (n & 31)) ? (1u << (n & 31)) - 1u : 0xffffffffu;
    __threadfence();
    __syncthreads();

    // ---- greedy cover (recmap.py:324-353)
    int n_ch = 0;
    while (n_ch < n_vrf && 0.0 < min_cover) {
        unsigned long long best = 0ull;
        for (int c = tid; c < n_cand; c += 256) {
            bool taken = false;
            for (int k = 0; k < n_ch; ++k) taken |= s_chosen[k] == c;
            if (taken) continue;
            int gain = 0;
            for (int w = 0; w < words; ++w) gain += __popc(ld_agent(mask + (size_t)c * words + w) & unobs[w]);
            const unsigned long long key = ((unsigned long long)(unsigned)gain << 32) | (unsigned)(0x7fffffff - c);
            best = key > best ? key : best;
        }
        best = block_max_u64<4>(best, s_u64);      // the largest gain, then the first candidate
        if (best == 0ull) break;
        const int c = 0x7fffffff - (int)(best & 0xffffffffu), gain = (int)(best >> 32);
        if (tid == 0) s_chosen[n_ch] = c;
        int rem = 0;
        for (int w = tid; w < words; w += 256) {
            const unsigned u = unobs[w] & ~ld_agent(mask + (size_t)c * words + w);
            unobs[w] = u;
            rem += __popc(u);
        }
        rem = block_sum_i32<4>(rem, s_i4);
        ++n_ch;
        if ((double)gain / (double)n < gain_floor) break;
        if (!(1.0 - (double)rem / (double)n < min_cover)) break;
    }

    // ---- recmap.py:369-403: a chosen frame stays when a point of the list that the table holds, with id >= 0, is a row of the
    // frame and projects inside the image
    int kept = 0;
    for (int k = 0; k < n_ch; ++k) {
        const int f = cand[s_chosen[k]];
        if (tid == 0) s_flag = 0;
        __syncthreads();
        const double* cam = frame_cams + (size_t)f * PRAM_MAPBUILD_CAM_COLS;
        const double qw = cam[0], qx = cam[1], qy = cam[2], qz = cam[3], tx = cam[4], ty = cam[5], tz = cam[6];
        const double fx = cam[7], fy = cam[8], cx = cam[9], cy = cam[10], im_w = cam[11], im_h = cam[12];
        const double r00 = 1.0 - 2.0 * qy * qy - 2.0 * qz * qz, r01 = 2.0 * qx * qy - 2.0 * qw * qz, r02 = 2.0 * qz * qx + 2.0 * qw * qy;
        const double r10 = 2.0 * qx * qy + 2.0 * qw * qz, r11 = 1.0 - 2.0 * qx * qx - 2.0 * qz * qz, r12 = 2.0 * qy * qz - 2.0 * qw * qx;
        const double r20 = 2.0 * qz * qx - 2.0 * qw * qy, r21 = 2.0 * qy * qz + 2.0 * qw * qx, r22 = 1.0 - 2.0 * qx * qx - 2.0 * qy * qy;
        int r0, r1;
        clamped_range(frame_off[f], frame_off[f + 1], n_rows, r0, r1);
        int flag = 0;
        for (int r = r0 + tid; r < r1; r += 256) {
            const long long id = ids[r];
            if (id < 0) continue;
            if (id == 0 ? s_has_zero == 0 : vrf_lookup(hkey, hpos, h, id) < 0) continue;
            const int lo = lower_bound_i64(pt_ids, n_points, id);
            if (lo >= n_points || pt_ids[lo] != id) continue;
            flag |= 1;
            const double x = pt_xyz[(size_t)lo * 3], y = pt_xyz[(size_t)lo * 3 + 1], z = pt_xyz[(size_t)lo * 3 + 2];
            const double X = r00 * x + r01 * y + r02 * z + tx, Y = r10 * x + r11 * y + r12 * z + ty, Z = r20 * x + r21 * y + r22 * z + tz;
            const double u = (fx * X + cx * Z) / Z, v = (fy * Y + cy * Z) / Z;
            if (u >= 0.0 && u < im_w && v >= 0.0 && v < im_h) flag |= 2;
        }
        if (flag) atomicOr(&s_flag, flag);
        __syncthreads();
        const bool keep = (s_flag & 2) != 0;
        if (keep && tid == 0) out[kept] = f;
        kept += keep;
        __syncthreads();
    }
    for (int k = kept + tid; k < n_vrf; k += 256) out[k] = -1;
    if (tid == 0) lm_vrf_n[l] = kept;
}

// the sections of pram_mapbuild_select_frames' workspace, 64-bit ones first
struct VrfLayout { size_t lf, hn, wn, bytes; };

static VrfLayout vrf_layout(int n_landmarks, int n_lm_points, int n_frames) {
    VrfLayout v;
    v.lf = (size_t)n_landmarks * (size_t)n_frames;
    v.hn = 2 * (size_t)n_lm_points + (size_t)n_landmarks;
    v.wn = ((size_t)n_lm_points >> 5) + (size_t)n_landmarks;
    v.bytes = 8 * (2 * v.lf + v.hn) + 4 * (2 * v.lf + v.hn + v.wn * (size_t)n_frames + v.wn + (size_t)n_frames);
    return v;
}

// entries of the tracks longer than the short path: the workspace covers trk_off up to the last of them
static long long desc_long_end(const int* trk_off_host, int n_points) {
    long long end = 0;
    for (int p = 0; p < n_points; ++p)
        if (trk_off_host[p + 1] - trk_off_host[p] > MB_SHORT) end = trk_off_host[p + 1];
    return end;
}

static bool offsets_ok(const int* off, int n) {
    if (off[0] != 0) return false;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

}  // namespace

extern "C" size_t pram_mapbuild_desc_workspace_bytes(const int* trk_off_host, int n_points) {
    if (trk_off_host == nullptr || n_points <= 0 || !offsets_ok(trk_off_host, n_points)) return 0;
    return (size_t)desc_long_end(trk_off_host, n_points) * 12;
}

extern "C" int pram_mapbuild_assign_descriptors(const float* descriptors, const int* frame_off, int n_frames, int n_rows, const int* trk_off,
                                                const int* trk_off_host, const int* trk_frame, const int* trk_kpt, int n_points,
                                                void* workspace, size_t workspace_bytes, float* pt_desc, int* pt_choice, void* stream) {
    PRAM_REQUIRE(descriptors && frame_off && trk_off && trk_off_host && trk_frame && trk_kpt && pt_desc && pt_choice,
                 "pram_mapbuild_assign_descriptors: null pointer");
    PRAM_REQUIRE(aligned(descriptors, 16) && aligned(pt_desc, 16), "pram_mapbuild_assign_descriptors: descriptors and pt_desc must be 16-byte aligned");
    PRAM_REQUIRE(aligned(frame_off, 4) && aligned(trk_off, 4) && aligned(trk_frame, 4) && aligned(trk_kpt, 4) && aligned(pt_choice, 4) &&
                 aligned(workspace, 8), "pram_mapbuild_assign_descriptors: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 0 && n_rows >= 0 && n_points >= 0, "pram_mapbuild_assign_descriptors: needs n_frames >= 0, n_rows >= 0, n_points >= 0");
    if (n_points == 0) return PRAM_OK;
    PRAM_REQUIRE(offsets_ok(trk_off_host, n_points), "pram_mapbuild_assign_descriptors: trk_off must start at 0 and not decrease");
    const long long end = desc_long_end(trk_off_host, n_points);
    PRAM_REQUIRE(workspace_bytes >= (size_t)end * 12 && (end == 0 || workspace != nullptr),
                 "pram_mapbuild_assign_descriptors: workspace of %zu bytes, needs %zu (pram_mapbuild_desc_workspace_bytes)", workspace_bytes,
                 (size_t)end * 12);
    double* ws_d = static_cast<double*>(workspace);
    int* ws_row = reinterpret_cast<int*>(ws_d + end);
    hipLaunchKernelGGL(mapbuild_desc_kernel, dim3(n_points), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(descriptors),
                       frame_off, n_frames, n_rows, trk_off, trk_frame, trk_kpt, trk_off_host[n_points], end, ws_d, ws_row,
                       reinterpret_cast<float4*>(pt_desc), pt_choice);
    return pram_launch_status("pram_mapbuild_assign_descriptors");
}

extern "C" size_t pram_mapbuild_vrf_workspace_bytes(int n_landmarks, int n_lm_points, int n_frames) {
    if (n_landmarks <= 0 || n_lm_points < 0 || n_frames < 0) return 0;
    return vrf_layout(n_landmarks, n_lm_points, n_frames).bytes;
}

extern "C" int pram_mapbuild_select_frames(const long long* point3d_ids, const int* frame_off, int n_frames, int n_rows, const long long* pt_ids,
                                           const int* pt_off, const int* pt_frames, int n_points, int n_entries, const double* pt_xyz,
                                           const int* lm_off, const int* lm_off_host, const long long* lm_points, int n_landmarks,
                                           const int* frame_ignored, const double* frame_cams, int min_obs, int topk_imgs, int n_vrf,
                                           double min_cover_ratio, double gain_floor, void* workspace, size_t workspace_bytes, int* lm_vrf,
                                           int* lm_vrf_n, void* stream) {
    PRAM_REQUIRE(point3d_ids && frame_off && pt_ids && pt_off && pt_frames && pt_xyz && lm_off && lm_off_host && lm_points && frame_ignored &&
                 frame_cams && workspace && lm_vrf && lm_vrf_n, "pram_mapbuild_select_frames: null pointer");
    PRAM_REQUIRE(aligned(point3d_ids, 8) && aligned(pt_ids, 8) && aligned(pt_xyz, 8) && aligned(lm_points, 8) && aligned(frame_cams, 8) &&
                 aligned(workspace, 8), "pram_mapbuild_select_frames: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(frame_off, 4) && aligned(pt_off, 4) && aligned(pt_frames, 4) && aligned(lm_off, 4) && aligned(frame_ignored, 4) &&
                 aligned(lm_vrf, 4) && aligned(lm_vrf_n, 4), "pram_mapbuild_select_frames: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 0 && n_rows >= 0 && n_points >= 0 && n_entries >= 0 && n_landmarks >= 0,
                 "pram_mapbuild_select_frames: needs n_frames >= 0, n_rows >= 0, n_points >= 0, n_entries >= 0, n_landmarks >= 0");
    PRAM_REQUIRE(topk_imgs >= 1 && n_vrf >= 1 && n_vrf <= MB_MAX_VRF, "pram_mapbuild_select_frames: needs topk_imgs >= 1 and 1 <= n_vrf <= %d", MB_MAX_VRF);
    if (n_landmarks == 0) return PRAM_OK;
    PRAM_REQUIRE(offsets_ok(lm_off_host, n_landmarks), "pram_mapbuild_select_frames: lm_off must start at 0 and not decrease");
    const int n_lm_points = lm_off_host[n_landmarks];
    PRAM_REQUIRE(n_lm_points < (1 << 30), "pram_mapbuild_select_frames: more than 2^30 landmark points");
    const VrfLayout v = vrf_layout(n_landmarks, n_lm_points, n_frames);
    PRAM_REQUIRE(workspace_bytes >= v.bytes, "pram_mapbuild_select_frames: workspace of %zu bytes, needs %zu (pram_mapbuild_vrf_workspace_bytes)",
                 workspace_bytes, v.bytes);
    VrfWs ws;
    ws.enc = static_cast<unsigned long long*>(workspace);
    ws.ekey = ws.enc + v.lf;
    ws.hkey = ws.ekey + v.lf;
    ws.cand = reinterpret_cast<int*>(ws.hkey + v.hn);
    ws.efr = ws.cand + v.lf;
    ws.hpos = ws.efr + v.lf;
    ws.mask = reinterpret_cast<unsigned*>(ws.hpos + v.hn);
    ws.unobs = ws.mask + v.wn * (size_t)n_frames;
    ws.fcount = reinterpret_cast<int*>(ws.unobs + v.wn);
    hipStream_t st = (hipStream_t)stream;
    // first encounter: all ones (no frame yet); hash keys 0 (empty; only ids > 0 are inserted), positions INT_MAX; masks 0
    bool ok = true;
    if (v.lf) ok = ok && hipMemsetD32Async((hipDeviceptr_t)ws.enc, (int)0xffffffff, 2 * v.lf, st) == hipSuccess;
    ok = ok && hipMemsetD32Async((hipDeviceptr_t)ws.hkey, 0, 2 * v.hn, st) == hipSuccess;
    ok = ok && hipMemsetD32Async((hipDeviceptr_t)ws.hpos, 0x7fffffff, v.hn, st) == hipSuccess;
    if (n_frames) ok = ok && hipMemsetD32Async((hipDeviceptr_t)ws.mask, 0, v.wn * (size_t)n_frames, st) == hipSuccess;
    if (!ok) return pram_launch_status("pram_mapbuild_select_frames");
    if (n_frames) hipLaunchKernelGGL(mapbuild_frame_obs_kernel, dim3(n_frames), dim3(256), 0, st, point3d_ids, frame_off, n_rows, ws.fcount);
    hipLaunchKernelGGL(mapbuild_vrf_kernel, dim3(n_landmarks), dim3(256), 0, st, point3d_ids, frame_off, n_frames, n_rows, pt_ids, pt_off,
                       pt_frames, n_points, n_entries, pt_xyz, lm_off, lm_points, n_lm_points, frame_ignored, frame_cams, min_obs, topk_imgs,
                       n_vrf, min_cover_ratio, gain_floor, ws, lm_vrf, lm_vrf_n);
    return pram_launch_status("pram_mapbuild_select_frames");
}
