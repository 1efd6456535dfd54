// A map's points from pairwise matches and known poses (what localization/triangulation.py of the reference hands to COLMAP):
// normalised keypoints, the epipolar test of every match, connected components over the kept matches, the CSR table of tracks and
// one robust multi-view solve per track.  float64 throughout; every sum runs per lane in ascending entry order and is combined by
// the butterfly of workgroup.h's wave_sum_f64, so a result does not depend on the launch or the run.  DESIGN.md 4.21 has the formulas and the
// deviations from COLMAP's incremental triangulator.
#include "obs.h"
#include "glue.h"
#include <math.h>

namespace {

constexpr int UNDISTORT_STEPS = PRAM_POSE_UNDISTORT_STEPS;
constexpr int GN_STEPS = PRAM_TRI_GN_STEPS;
constexpr int SCAN = 256;                    // rows per block of the scan over labels

// the frame f with frame_off[f] <= r < frame_off[f + 1] (frames may be empty), never beyond n_frames - 1
__device__ __forceinline__ int frame_of_row(const int* __restrict__ frame_off, int n_frames, int r) {
    return first_true(0, n_frames - 1, [&](int f) { return frame_off[f + 1] > r; });
}

// ---------------------------------------------------------------- the frame table
__global__ __launch_bounds__(64) void tri_frames_kernel(const double* __restrict__ qvec, const double* __restrict__ tvec,
                                                        const int* __restrict__ cam_model, const double* __restrict__ cam_params, int n_frames,
                                                        double* __restrict__ table) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n_frames) return;
    const double* q = qvec + (size_t)f * 4;
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double qw = q[0] / nq, qx = q[1] / nq, qy = q[2] / nq, qz = q[3] / nq;
    const double tx = tvec[(size_t)f * 3], ty = tvec[(size_t)f * 3 + 1], tz = tvec[(size_t)f * 3 + 2];
    double* T = table + (size_t)f * FC;
    T[0] = 1.0 - 2.0 * qy * qy - 2.0 * qz * qz; T[1] = 2.0 * qx * qy - 2.0 * qw * qz; T[2] = 2.0 * qz * qx + 2.0 * qw * qy;
    T[3] = 2.0 * qx * qy + 2.0 * qw * qz; T[4] = 1.0 - 2.0 * qx * qx - 2.0 * qz * qz; T[5] = 2.0 * qy * qz - 2.0 * qw * qx;
    T[6] = 2.0 * qz * qx - 2.0 * qw * qy; T[7] = 2.0 * qy * qz + 2.0 * qw * qx; T[8] = 1.0 - 2.0 * qx * qx - 2.0 * qy * qy;
    T[9] = tx; T[10] = ty; T[11] = tz;
    T[12] = -(T[0] * tx + T[3] * ty + T[6] * tz);
    T[13] = -(T[1] * tx + T[4] * ty + T[7] * tz);
    T[14] = -(T[2] * tx + T[5] * ty + T[8] * tz);
    const Cam c = cam_unify(cam_model[f], cam_params + (size_t)f * PRAM_POSE_CAM_PARAMS);
    T[15] = (c.fx + c.fy) / 2.0;
}

// ---------------------------------------------------------------- normalise: pixels -> normalised camera plane, once per table
__global__ __launch_bounds__(256) void tri_normalize_kernel(const float* __restrict__ kpts, const int* __restrict__ frame_off,
                                                            const int* __restrict__ cam_model, const double* __restrict__ cam_params,
                                                            int n_frames, int n_rows, double off, double* __restrict__ norm) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const int f = frame_of_row(frame_off, n_frames, r);
    const Cam c = cam_unify(cam_model[f], cam_params + (size_t)f * PRAM_POSE_CAM_PARAMS);
    const double xd = (((double)kpts[(size_t)r * 2] + off) - c.cx) / c.fx, yd = (((double)kpts[(size_t)r * 2 + 1] + off) - c.cy) / c.fy;
    double u = xd, v = yd;
    for (int it = 0; it < UNDISTORT_STEPS; ++it) {
        double fu, fv, j11, j12, j22;
        distort(c, u, v, fu, fv);
        fu -= xd; fv -= yd;
        distort_jac(c, u, v, j11, j12, j22);
        const double det = j11 * j22 - j12 * j12;
        if (fabs(det) > 1e-12) {
            const double su = (j22 * fu - j12 * fv) / det, sv = (j11 * fv - j12 * fu) / det;
            u -= su; v -= sv;
        }
    }
    norm[(size_t)r * 2] = u; norm[(size_t)r * 2 + 1] = v;
}

// ---------------------------------------------------------------- verify: one workgroup per pair, ordered compaction
__global__ __launch_bounds__(256) void tri_verify_kernel(const double* __restrict__ norm, const int* __restrict__ frame_off,
                                                         const int* __restrict__ pairs, const int* __restrict__ m_off,
                                                         const int* __restrict__ matches, const double* __restrict__ table, int n_frames,
                                                         int n_matches, double max_error, unsigned char* __restrict__ keep,
                                                         int* __restrict__ kept, int* __restrict__ edges, int* __restrict__ count) {
    __shared__ int wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int f0 = pairs[(size_t)p * 2], f1 = pairs[(size_t)p * 2 + 1];
    int m0, m1;
    clamped_range(m_off[p], m_off[p + 1], n_matches, m0, m1);
    const bool okp = f0 >= 0 && f0 < n_frames && f1 >= 0 && f1 < n_frames;      // uniform
    int r0 = 0, r1 = 0, n0 = 0, n1 = 0;
    double E[9], th0 = 0.0, th1 = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) E[a] = 0.0;
    if (okp) {
        r0 = frame_off[f0]; n0 = frame_off[f0 + 1] - r0;
        r1 = frame_off[f1]; n1 = frame_off[f1 + 1] - r1;
        const double* A = table + (size_t)f0 * FC;
        const double* B = table + (size_t)f1 * FC;
        double R[9];      // cam1_from_cam0: R = R1 R0^T, t = t1 - R t0
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) R[a * 3 + c] = B[a * 3] * A[c * 3] + B[a * 3 + 1] * A[c * 3 + 1] + B[a * 3 + 2] * A[c * 3 + 2];
        const double tx = B[9] - (R[0] * A[9] + R[1] * A[10] + R[2] * A[11]);
        const double ty = B[10] - (R[3] * A[9] + R[4] * A[10] + R[5] * A[11]);
        const double tz = B[11] - (R[6] * A[9] + R[7] * A[10] + R[8] * A[11]);
        const double nt = sqrt(tx * tx + ty * ty + tz * tz);      // 0: E is NaN, every match of the pair is dropped
        const double x = tx / nt, y = ty / nt, z = tz / nt;
        for (int c = 0; c < 3; ++c) {      // E = [t / |t|]x R
            E[c] = y * R[6 + c] - z * R[3 + c];
            E[3 + c] = z * R[c] - x * R[6 + c];
            E[6 + c] = x * R[3 + c] - y * R[c];
        }
        th0 = max_error / A[15]; th1 = max_error / B[15];
    }
    int base = 0;
    for (int c0 = m0; c0 < m1; c0 += 256) {
        const int e = c0 + tid;
        bool k = false;
        int i0 = -1, i1 = -1;
        if (e < m1) {
            i0 = matches[(size_t)e * 2]; i1 = matches[(size_t)e * 2 + 1];
            if (okp && i0 >= 0 && i0 < n0 && i1 >= 0 && i1 < n1) {      // an index outside its frame is never dereferenced
                const double u0 = norm[(size_t)(r0 + i0) * 2], v0 = norm[(size_t)(r0 + i0) * 2 + 1];
                const double u1 = norm[(size_t)(r1 + i1) * 2], v1 = norm[(size_t)(r1 + i1) * 2 + 1];
                const double lj0 = E[0] * u0 + E[1] * v0 + E[2], lj1 = E[3] * u0 + E[4] * v0 + E[5];
                const double li0 = E[0] * u1 + E[3] * v1 + E[6], li1 = E[1] * u1 + E[4] * v1 + E[7], li2 = E[2] * u1 + E[5] * v1 + E[8];
                const double dist = fabs(u0 * li0 + v0 * li1 + li2);
                const double e0 = dist / sqrt(li0 * li0 + li1 * li1), e1 = dist / sqrt(lj0 * lj0 + lj1 * lj1);
                k = e0 <= th0 && e1 <= th1;      // NaN compares false
            }
            keep[e] = k;
            edges[(size_t)e * 2] = k ? r0 + i0 : -1; edges[(size_t)e * 2 + 1] = k ? r1 + i1 : -1;
        }
        int total;
        const int o = chunk_offset<4>(k, wsum, total);
        if (k) { kept[(size_t)(m0 + base + o) * 2] = i0; kept[(size_t)(m0 + base + o) * 2 + 1] = i1; }
        base += total;
    }
    if (tid == 0) count[p] = base;
}

// ---------------------------------------------------------------- components: hook to the smaller root, jump, until nothing hooks
// state: [0] a hook happened this round, [1] done, [2] rounds run.  A label only ever decreases and always names a row of the same
// component, so whatever order the atomics land in, the fixed point labels every row with its component's smallest row.
__global__ __launch_bounds__(256) void tri_cc_init_kernel(int* __restrict__ label, int n_rows, int* __restrict__ state) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < n_rows) label[x] = x;
    if (x < PRAM_TRI_CC_STATE_WORDS) state[x] = 0;
}

__global__ __launch_bounds__(256) void tri_cc_hook_kernel(const int* __restrict__ edges, int n_edges, int n_rows, int* label, int* state) {
    if (state[1]) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[(size_t)e * 2], v = edges[(size_t)e * 2 + 1];
    if (u < 0 || v < 0 || u >= n_rows || v >= n_rows) return;
    const int ru = label[u], rv = label[v];
    if (ru != rv) {
        atomicMin(&label[ru > rv ? ru : rv], ru > rv ? rv : ru);
        state[0] = 1;
    }
}

__global__ __launch_bounds__(256) void tri_cc_jump_kernel(int* label, int n_rows, const int* __restrict__ state) {
    if (state[1]) return;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n_rows) return;
    int l = label[x];
    for (int it = 0; it < n_rows; ++it) {      // labels strictly decrease along a chain
        const int nl = label[l];
        if (nl == l) break;
        l = nl;
    }
    label[x] = l;
}

__global__ void tri_cc_end_kernel(int* __restrict__ state) {
    if (state[1]) return;
    if (!state[0]) state[1] = 1;
    state[0] = 0;
    state[2] += 1;
}

// ---------------------------------------------------------------- the two-level exclusive scan the tracks and the adjacency share
// A user U names its NV running sums: terms() makes them of a position's count, local[q] takes sum q, and finish() is what thread
// 0 of level 2 does with the totals.  Level 1 leaves position x's offset inside its block at local[q][x] and the block's total
// at bsum[blk * NV + q]; level 2 (one workgroup) turns the totals into the blocks' bases in place.  scan_offset() is how both
// users read the result.  The workspace: per row a count and a fill cursor (adjacent: one memset clears both), the blocks' sums,
// then what only the user has.
struct ScanWs { int* count; int* cursor; int* bsum; int* rest; };

struct TrackScan {      // of a label's size: is it a track, and its entries; the totals are the table's sizes and trk_off's last entry
    static constexpr int NV = 2;
    int* local[2]; int* sizes; int* trk_off;
    __device__ static void terms(int s, int* v) { v[0] = s >= 2 ? 1 : 0; v[1] = s >= 2 ? s : 0; }
    __device__ void finish(const int* total) const { sizes[0] = total[0]; sizes[1] = total[1]; trk_off[total[0]] = total[1]; }
};

struct AdjScan {      // a row's degree; segments = n_rows is what the sort reads as its number of lists
    static constexpr int NV = 1;
    int* local[1]; int* segments; int n_rows;
    __device__ static void terms(int s, int* v) { v[0] = s; }
    __device__ void finish(const int*) const { segments[0] = n_rows; }
};

// positions 0 .. n_out - 1; a position beyond n_in counts 0 (the adjacency's last stands for the total)
template <class U>
__global__ __launch_bounds__(SCAN) void tri_scan_blocks_kernel(const int* __restrict__ count, int n_in, int n_out, U u, int* __restrict__ bsum) {
    __shared__ int wsum[4];
    const int x = blockIdx.x * SCAN + threadIdx.x;
    int v[U::NV];
    U::terms(x < n_in ? count[x] : 0, v);
#pragma unroll
    for (int q = 0; q < U::NV; ++q) {
        int total;
        const int o = chunk_offset_n<4>(v[q], wsum, total);
        if (x < n_out) u.local[q][x] = o;
        if (threadIdx.x == 0) bsum[(size_t)blockIdx.x * U::NV + q] = total;
    }
}

template <class U>
__global__ __launch_bounds__(256) void tri_scan_totals_kernel(int* __restrict__ bsum, int n_blocks, U u) {
    __shared__ int wsum[4];
    int base[U::NV];
#pragma unroll
    for (int q = 0; q < U::NV; ++q) base[q] = 0;
    for (int c0 = 0; c0 < n_blocks; c0 += 256) {
        const int i = c0 + threadIdx.x;
#pragma unroll
        for (int q = 0; q < U::NV; ++q) {
            int total;
            const int o = chunk_offset_n<4>(i < n_blocks ? bsum[(size_t)i * U::NV + q] : 0, wsum, total);
            if (i < n_blocks) bsum[(size_t)i * U::NV + q] = base[q] + o;
            base[q] += total;
        }
    }
    if (threadIdx.x == 0) u.finish(base);
}

// sum q at position x: the offset inside its block + the block's base
template <int NV>
__device__ __forceinline__ int scan_offset(const int* local, const int* bsum, int x, int q) {
    return local[x] + bsum[(size_t)(x / SCAN) * NV + q];
}

// ---------------------------------------------------------------- tracks: counts, the scan over labels, a cursor fill, a sort per track
__global__ __launch_bounds__(256) void tri_count_kernel(const int* __restrict__ label, int n_rows, int* __restrict__ size) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n_rows) return;
    const int l = label[x];
    if (l >= 0 && l < n_rows) atomicAdd(&size[l], 1);
}

__global__ __launch_bounds__(256) void tri_fill_kernel(const int* __restrict__ label, ScanWs ws, TrackScan u, int n_rows,
                                                       int* __restrict__ trk_label, int* __restrict__ trk_row) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n_rows) return;
    const int l = label[x];
    if (l < 0 || l >= n_rows || ws.count[l] < 2) return;
    const int t = scan_offset<2>(u.local[0], ws.bsum, l, 0), eo = scan_offset<2>(u.local[1], ws.bsum, l, 1);
    const int pos = atomicAdd(&ws.cursor[l], 1);
    if (eo + pos < n_rows) trk_row[eo + pos] = x;
    if (x == l) { u.trk_off[t] = eo; trk_label[t] = l; }
}

// One wave per track: a bitonic network in its flip form (every comparator ascending, so the positions beyond the track's length
// stand for +inf and are skipped), in place in global memory; no cap on the length.
__global__ __launch_bounds__(64) void tri_sort_kernel(const int* __restrict__ sizes, const int* __restrict__ trk_off, int* trk_row, int n_rows) {
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= sizes[0]) return;
    int beg, end;
    clamped_range(trk_off[t], trk_off[t + 1], n_rows, beg, end);
    const int L = end - beg;
    int* a = trk_row + beg;
    int N2 = 1;
    for (int it = 0; it < 31 && N2 < L; ++it) N2 <<= 1;
    for (int k = 2; k <= N2; k <<= 1) {
        const int h = k >> 1;
        for (int i = lane; i < (N2 >> 1); i += 64) {
            const int blk = i / h, w = i - blk * h, lo = blk * k + w, hi = blk * k + k - 1 - w;
            if (hi < L) { const int x = a[lo], y = a[hi]; if (x > y) { a[lo] = y; a[hi] = x; } }
        }
        __syncthreads();
        for (int j = k >> 2; j >= 1; j >>= 1) {
            for (int i = lane; i < (N2 >> 1); i += 64) {
                const int blk = i / j, lo = blk * 2 * j + (i - blk * j), hi = lo + j;
                if (hi < L) { const int x = a[lo], y = a[hi]; if (x > y) { a[lo] = y; a[hi] = x; } }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void tri_derive_kernel(const int* __restrict__ sizes, const int* __restrict__ trk_row,
                                                         const int* __restrict__ frame_off, int n_frames, int n_rows,
                                                         int* __restrict__ trk_frame, int* __restrict__ trk_kpt) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= sizes[1] || e >= n_rows) return;
    const int r = trk_row[e];
    const int f = frame_of_row(frame_off, n_frames, r);
    trk_frame[e] = f; trk_kpt[e] = r - frame_off[f];
}

// ---------------------------------------------------------------- triangulate: one wave per track
// entry e's row and frame; ok: the tables hold both (a caller's own track table may name neither)
struct Entry { int r, f; bool ok; };

__global__ __launch_bounds__(64) void tri_triangulate_kernel(Obs g, const int* __restrict__ trk_off, const int* __restrict__ trk_label,
                                                             const int* __restrict__ trk_row, const int* __restrict__ trk_frame,
                                                             int n_entries, int trials, unsigned long long seed, double min_angle,
                                                             double max_err, int* __restrict__ accept, double* __restrict__ xyz,
                                                             double* __restrict__ err, int* __restrict__ kept_n, int* __restrict__ best,
                                                             unsigned char* ent_keep, double* ent_err) {
    const int t = blockIdx.x, lane = threadIdx.x;
    int beg, end;
    clamped_range(trk_off[t], trk_off[t + 1], n_entries, beg, end);
    const int L = end - beg;
    const auto entry = [&](int e) -> Entry {
        const int r = trk_row[e], f = trk_frame[e];
        return {r, f, r >= 0 && r < g.n_rows && f >= 0 && f < g.n_frames};
    };
    const auto inlier = [&](int e, V3 X, double thr2, double& err2) {
        const Entry en = entry(e);
        err2 = 0.0;
        return en.ok && obs_inlier(g, en.r, en.f, X, thr2, err2);
    };
    const double thr2 = max_err * max_err;
    const long long all = (long long)L * (L - 1) / 2;
    const bool exhaustive = all <= (long long)trials;
    const int H = exhaustive ? (int)all : trials;
    const unsigned long long key0 = sm64(seed) ^ ((unsigned long long)(unsigned)trk_label[t] << 32);

    // ---- hypotheses: every value below is uniform over the wave
    int bc = 0, bh = -1, hi_ = 0, hj_ = 1;
    double bs = 0.0;
    V3 bX = {0.0, 0.0, 0.0};
    for (int h = 0; h < H; ++h) {
        int i, j;
        if (exhaustive) {
            i = hi_; j = hj_;
            if (++hj_ == L) { ++hi_; hj_ = hi_ + 1; }
        } else {
            const unsigned long long key = sm64(key0 ^ (unsigned long long)(unsigned)h);
            int a = (int)__umul64hi(sm64(key + 0ull), (unsigned long long)L);
            int b = (int)__umul64hi(sm64(key + 1ull), (unsigned long long)(L - 1));
            b += b >= a;
            i = a < b ? a : b; j = a < b ? b : a;
        }
        const Entry ei = entry(beg + i), ej = entry(beg + j);
        if (!ei.ok || !ej.ok || ei.f == ej.f) continue;
        const V3 C1 = obs_centre(g, ei.f), C2 = obs_centre(g, ej.f), d1 = obs_ray(g, ei.r, ei.f), d2 = obs_ray(g, ej.r, ej.f);
        if (!(angle(d1, d2) >= min_angle)) continue;
        const V3 X = ray_midpoint(C1, d1, C2, d2);
        if (!(obs_depth(g, ei.f, X) > 0.0) || !(obs_depth(g, ej.f, X) > 0.0)) continue;
        int cnt = 0;
        double sse = 0.0;
        for (int k = lane; k < L; k += 64) {
            double e2;
            const bool in = inlier(beg + k, X, thr2, e2);
            cnt += in;
            sse += in ? e2 : 0.0;
        }
        cnt = wave_sum_i32(cnt);
        sse = wave_sum_f64(sse);
        if (cnt >= 2 && (cnt > bc || (cnt == bc && sse < bs))) { bc = cnt; bs = sse; bh = h; bX = X; }      // the lower index keeps a tie
    }
    if (bh < 0) {
        for (int k = lane; k < L; k += 64) { ent_keep[beg + k] = 0; ent_err[beg + k] = -1.0; }
        if (lane == 0) {
            accept[t] = 0; kept_n[t] = 0; best[t] = -1; err[t] = 0.0;
            xyz[(size_t)t * 3] = 0.0; xyz[(size_t)t * 3 + 1] = 0.0; xyz[(size_t)t * 3 + 2] = 0.0;
        }
        return;
    }

    // ---- refit on the winner's inliers (ent_keep holds them until the final marking; a lane reads back its own entries only)
    V3 X = bX;
    {
        double acc[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) acc[q] = 0.0;
        for (int k = lane; k < L; k += 64) {
            double e2;
            const bool in = inlier(beg + k, bX, thr2, e2);
            ent_keep[beg + k] = in;
            if (!in) continue;
            const Entry en = entry(beg + k);
            const V3 dd = obs_ray(g, en.r, en.f), C = obs_centre(g, en.f);
            const double m00 = 1.0 - dd.x * dd.x, m01 = -dd.x * dd.y, m02 = -dd.x * dd.z, m11 = 1.0 - dd.y * dd.y, m12 = -dd.y * dd.z,
                         m22 = 1.0 - dd.z * dd.z;
            acc[0] += m00; acc[1] += m01; acc[2] += m02; acc[3] += m11; acc[4] += m12; acc[5] += m22;
            acc[6] += m00 * C.x + m01 * C.y + m02 * C.z;
            acc[7] += m01 * C.x + m11 * C.y + m12 * C.z;
            acc[8] += m02 * C.x + m12 * C.y + m22 * C.z;
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) acc[q] = wave_sum_f64(acc[q]);
        double x[3];
        if (chol_solve3(acc, acc + 6, x)) X = {x[0], x[1], x[2]};
    }
    for (int it = 0; it < GN_STEPS; ++it) {
        double acc[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) acc[q] = 0.0;
        for (int k = lane; k < L; k += 64) {
            if (!ent_keep[beg + k]) continue;
            double z, r0, r1, J[6];
            obs_residual(g, trk_row[beg + k], trk_frame[beg + k], X, z, r0, r1, true, J);
            if (!(z > 1e-12) || !fin(r0 * r0 + r1 * r1)) continue;
            acc[0] += J[0] * J[0] + J[3] * J[3]; acc[1] += J[0] * J[1] + J[3] * J[4]; acc[2] += J[0] * J[2] + J[3] * J[5];
            acc[3] += J[1] * J[1] + J[4] * J[4]; acc[4] += J[1] * J[2] + J[4] * J[5]; acc[5] += J[2] * J[2] + J[5] * J[5];
            acc[6] -= J[0] * r0 + J[3] * r1; acc[7] -= J[1] * r0 + J[4] * r1; acc[8] -= J[2] * r0 + J[5] * r1;
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) acc[q] = wave_sum_f64(acc[q]);
        double x[3];
        if (chol_solve3(acc, acc + 6, x)) X = {X.x + x[0], X.y + x[1], X.z + x[2]};
    }

    // ---- final marking at X, then one entry per frame: the smallest error, the lowest row on a tie (a frame's entries are adjacent)
    for (int k = lane; k < L; k += 64) {
        double e2;
        const bool in = inlier(beg + k, X, thr2, e2);
        ent_err[beg + k] = in ? sqrt(e2) : -1.0;
    }
    __syncthreads();
    int cnt = 0;
    double esum = 0.0;
    for (int k = lane; k < L; k += 64) {
        const double mine = ent_err[beg + k];
        bool keep = mine >= 0.0;
        if (keep) {
            const int f = trk_frame[beg + k];
            for (int o = k - 1; o >= 0 && trk_frame[beg + o] == f; --o) {
                const double other = ent_err[beg + o];
                if (other >= 0.0 && other <= mine) { keep = false; break; }
            }
            for (int o = k + 1; keep && o < L && trk_frame[beg + o] == f; ++o) {
                const double other = ent_err[beg + o];
                if (other >= 0.0 && other < mine) keep = false;
            }
        }
        ent_keep[beg + k] = keep;
        cnt += keep;
        esum += keep ? mine : 0.0;
    }
    cnt = wave_sum_i32(cnt);
    esum = wave_sum_f64(esum);
    __syncthreads();
    // ---- some pair of kept entries sees X under min_angle or more
    bool found = false;
    for (int k = lane; k < L && !found; k += 64) {
        if (!ent_keep[beg + k]) continue;
        const V3 vi = sub(X, obs_centre(g, trk_frame[beg + k]));
        for (int o = k + 1; o < L; ++o) {
            if (!ent_keep[beg + o]) continue;
            if (angle(vi, sub(X, obs_centre(g, trk_frame[beg + o]))) >= min_angle) { found = true; break; }
        }
    }
    const bool any = __any(found);
    if (lane == 0) {
        accept[t] = cnt >= 2 && any; kept_n[t] = cnt; best[t] = bh; err[t] = cnt > 0 ? esum / (double)cnt : 0.0;
        xyz[(size_t)t * 3] = X.x; xyz[(size_t)t * 3 + 1] = X.y; xyz[(size_t)t * 3 + 2] = X.z;
    }
}

// ---------------------------------------------------------------- stage 2b: the rows' adjacency and every edge's third-view support
// adjacency: degrees by integer atomics, the scan over rows 0 .. n_rows (straight into adj_off), a cursor fill, then
// tri_sort_kernel over adj_off, so that the table is a function of the edge set alone.  An edge counts when both ends are rows
// and differ.
__device__ __forceinline__ bool edge_ok(int u, int v, int n_rows) { return u >= 0 && v >= 0 && u < n_rows && v < n_rows && u != v; }

__global__ __launch_bounds__(256) void tri_adj_count_kernel(const int* __restrict__ edges, int n_edges, int n_rows, int* __restrict__ deg) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[(size_t)e * 2], v = edges[(size_t)e * 2 + 1];
    if (!edge_ok(u, v, n_rows)) return;
    atomicAdd(&deg[u], 1);
    atomicAdd(&deg[v], 1);
}

__global__ __launch_bounds__(256) void tri_adj_offsets_kernel(ScanWs ws, const int* __restrict__ frame_off, int n_frames, int n_rows,
                                                              int* __restrict__ adj_off, int* __restrict__ row_frame) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x > n_rows) return;
    adj_off[x] = scan_offset<1>(adj_off, ws.bsum, x, 0);
    if (x < n_rows) row_frame[x] = frame_of_row(frame_off, n_frames, x);
}

__global__ __launch_bounds__(256) void tri_adj_fill_kernel(const int* __restrict__ edges, int n_edges, int n_rows, ScanWs ws,
                                                           const int* __restrict__ adj_off, int* __restrict__ adj) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[(size_t)e * 2], v = edges[(size_t)e * 2 + 1];
    if (!edge_ok(u, v, n_rows)) return;
    const long long pu = (long long)adj_off[u] + atomicAdd(&ws.cursor[u], 1), pv = (long long)adj_off[v] + atomicAdd(&ws.cursor[v], 1);
    if (pu >= 0 && pu < 2ll * n_edges) adj[pu] = v;
    if (pv >= 0 && pv < 2ll * n_edges) adj[pv] = u;
}

// the adjacency as the support reads it; n: the entries adj holds
struct Adj { const int* off; const int* adj; const int* row_frame; int n; };

constexpr int SUP_WAVES = 4;      // edges per workgroup

// One wave per edge (u, v): the lanes stride over adj(u) followed by adj(v); a witness is a row of a third frame, counted once.
// Of the pairs (u, v), (u, w), (v, w) the one whose rays meet under the largest angle (the first on a tie) gives X; w confirms the
// edge when that angle reaches min_angle and u, v and w are inliers of X.  No LDS and no floating-point atomics.
__global__ __launch_bounds__(64 * SUP_WAVES) void tri_support_kernel(Obs g, Adj a, const int* __restrict__ edges, int n_edges, double min_angle,
                                                                     double max_err, int min_support, int* __restrict__ support,
                                                                     int* __restrict__ edges_out) {
    const int e = blockIdx.x * SUP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= n_edges) return;
    const int u = edges[(size_t)e * 2], v = edges[(size_t)e * 2 + 1];
    const double thr2 = max_err * max_err;
    int cnt = 0;
    bool ok = edge_ok(u, v, g.n_rows);
    int fu = -1, fv = -1;
    if (ok) {
        fu = a.row_frame[u]; fv = a.row_frame[v];
        ok = fu >= 0 && fu < g.n_frames && fv >= 0 && fv < g.n_frames && fu != fv;
    }
    if (ok) {      // uniform over the wave
        const V3 Cu = obs_centre(g, fu), Cv = obs_centre(g, fv), du = obs_ray(g, u, fu), dv = obs_ray(g, v, fv);
        const double a_uv = angle(du, dv);
        int bu, eu, bv, ev;      // the two lists, their offsets cut into the table
        clamped_range(a.off[u], a.off[u + 1], a.n, bu, eu);
        clamped_range(a.off[v], a.off[v + 1], a.n, bv, ev);
        const int nu = eu - bu, nv = ev - bv;
        const long long total = (long long)nu + nv;
        for (long long k = lane; k < total; k += 64) {
            int w;
            if (k < nu) {
                w = a.adj[bu + (int)k];
                if (k > 0 && a.adj[bu + (int)k - 1] == w) continue;
            } else {
                const int j = (int)(k - nu);
                w = a.adj[bv + j];
                if (j > 0 && a.adj[bv + j - 1] == w) continue;
                const int lo = first_true(0, nu, [&](int i) { return a.adj[bu + i] >= w; });      // adj(u) holds w already
                if (lo < nu && a.adj[bu + lo] == w) continue;
            }
            if (w < 0 || w >= g.n_rows || w == u || w == v) continue;
            const int fw = a.row_frame[w];
            if (fw < 0 || fw >= g.n_frames || fw == fu || fw == fv) continue;
            const V3 Cw = obs_centre(g, fw), dw = obs_ray(g, w, fw);
            const double a_uw = angle(du, dw), a_vw = angle(dv, dw);
            int pick = 0;
            double best = a_uv;
            if (a_uw > best) { pick = 1; best = a_uw; }
            if (a_vw > best) { pick = 2; best = a_vw; }
            if (!(best >= min_angle)) continue;
            const V3 X = pick == 0 ? ray_midpoint(Cu, du, Cv, dv) : (pick == 1 ? ray_midpoint(Cu, du, Cw, dw) : ray_midpoint(Cv, dv, Cw, dw));
            double e2;
            const bool iu = obs_inlier(g, u, fu, X, thr2, e2), iv = obs_inlier(g, v, fv, X, thr2, e2), iw = obs_inlier(g, w, fw, X, thr2, e2);
            cnt += iu && iv && iw;
        }
    }
    cnt = wave_sum_i32(cnt);
    if (lane == 0) {
        const bool keep = cnt >= min_support;
        support[e] = cnt;
        edges_out[(size_t)e * 2] = keep ? u : -1; edges_out[(size_t)e * 2 + 1] = keep ? v : -1;
    }
}

// ---------------------------------------------------------------- split: mark the rows a round used, keep the edges between free rows
constexpr unsigned char ROW_FREE = PRAM_TRI_ROW_FREE, ROW_TAKEN = PRAM_TRI_ROW_TAKEN, ROW_DEAD = PRAM_TRI_ROW_DEAD;

__global__ __launch_bounds__(256) void tri_split_init_kernel(unsigned char* __restrict__ state, int n_rows, int first, int* __restrict__ n_live) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (first && x < n_rows) state[x] = ROW_DEAD;
    if (x == 0) n_live[0] = 0;
}

// One thread per entry: its track is the last whose offset is not beyond it, track 0 when none is (an offset cut into
// [0, n_entries] compares with an entry as the offset itself does).  The search runs from the last track down, so the first
// index that holds is the last such track.  A row is in one track, so every byte has one writer.
__global__ __launch_bounds__(256) void tri_split_mark_kernel(const int* __restrict__ trk_off, const int* __restrict__ trk_row, int n_tracks,
                                                             int n_entries, const int* __restrict__ accept,
                                                             const unsigned char* __restrict__ entry_keep, int n_rows,
                                                             unsigned char* __restrict__ state) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_entries) return;
    const int last = n_tracks - 1;
    const int lo = last - first_true(0, last, [&](int j) { return trk_off[last - j] <= e; });
    int beg, end;
    clamped_range(trk_off[lo], trk_off[lo + 1], n_entries, beg, end);
    if (e < beg || e >= end) return;
    const int r = trk_row[e];
    if (r < 0 || r >= n_rows) return;
    state[r] = accept[lo] ? (entry_keep[e] ? ROW_TAKEN : ROW_FREE) : ROW_DEAD;
}

// One thread per edge; the survivors of a wave are counted by a ballot and added by its first lane.
__global__ __launch_bounds__(256) void tri_split_filter_kernel(const int* __restrict__ edges, int n_edges, int n_rows,
                                                               const unsigned char* __restrict__ state, int* __restrict__ edges_out,
                                                               int* n_live) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    bool live = false;
    if (e < n_edges) {
        const int u = edges[(size_t)e * 2], v = edges[(size_t)e * 2 + 1];
        live = u >= 0 && v >= 0 && u < n_rows && v < n_rows && state[u] == ROW_FREE && state[v] == ROW_FREE;
        edges_out[(size_t)e * 2] = live ? u : -1; edges_out[(size_t)e * 2 + 1] = live ? v : -1;
    }
    const int cnt = __popcll(__ballot(live));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_live, cnt);
}

int check_models(const int* cam_model_host, int n_frames, const char* what) {
    for (int f = 0; f < n_frames; ++f)
        if (cam_model_host[f] < PRAM_CAM_SIMPLE_PINHOLE || cam_model_host[f] > PRAM_CAM_OPENCV) {
            pram_set_error("%s: camera model id %d of frame %d is not supported", what, cam_model_host[f], f);
            return PRAM_E_UNSUPPORTED;
        }
    return PRAM_OK;
}

constexpr int MAX_ROWS = 1 << 30;      // the sort's network doubles a length

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// The scan's workspace for n_rows rows and n_bsum block sums, with rest_bytes behind for what only the user has.  Null: its size.
size_t row_stride(int n_rows) { return align_up((size_t)(n_rows > 0 ? n_rows : 1) * sizeof(int)); }

size_t carve_scan_ws(void* workspace, int n_rows, int n_bsum, size_t rest_bytes, ScanWs* ws) {
    const size_t stride = row_stride(n_rows), bsum = align_up((size_t)n_bsum * sizeof(int));
    char* w = static_cast<char*>(workspace);
    if (ws) *ws = {reinterpret_cast<int*>(w), reinterpret_cast<int*>(w + stride), reinterpret_cast<int*>(w + 2 * stride),
                   reinterpret_cast<int*>(w + 2 * stride + bsum)};
    return 2 * stride + bsum + rest_bytes;
}

// the tracks scan over n_rows positions, two sums a block; the adjacency over n_rows + 1, one
int track_blocks(int n_rows) { return cdiv(n_rows > 0 ? n_rows : 1, SCAN); }
int adj_blocks(int n_rows) { return cdiv(n_rows + 1, SCAN); }

}  // namespace

extern "C" int pram_tri_frames(const double* qvec, const double* tvec, const int* cam_model, const double* cam_params,
                               const int* cam_model_host, int n_frames, double* table, void* stream) {
    PRAM_REQUIRE(qvec && tvec && cam_model && cam_params && cam_model_host && table, "pram_tri_frames: null pointer");
    PRAM_REQUIRE(aligned(qvec, 8) && aligned(tvec, 8) && aligned(cam_model, 4) && aligned(cam_params, 8) && aligned(table, 8),
                 "pram_tri_frames: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 0, "pram_tri_frames: needs n_frames >= 0");
    const int rc = check_models(cam_model_host, n_frames, "pram_tri_frames");
    if (rc != PRAM_OK) return rc;
    if (n_frames == 0) return PRAM_OK;
    hipLaunchKernelGGL(tri_frames_kernel, dim3(cdiv(n_frames, 64)), dim3(64), 0, (hipStream_t)stream, qvec, tvec, cam_model, cam_params, n_frames,
                       table);
    return pram_launch_status("pram_tri_frames");
}

extern "C" int pram_tri_normalize(const float* keypoints, const int* frame_off, const int* cam_model, const double* cam_params,
                                  const int* cam_model_host, int n_frames, int n_rows, double pixel_offset, double* norm, void* stream) {
    PRAM_REQUIRE(keypoints && frame_off && cam_model && cam_params && cam_model_host && norm, "pram_tri_normalize: null pointer");
    PRAM_REQUIRE(aligned(keypoints, 4) && aligned(frame_off, 4) && aligned(cam_model, 4) && aligned(cam_params, 8) && aligned(norm, 8),
                 "pram_tri_normalize: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 0 && n_rows >= 0 && (n_rows == 0 || n_frames >= 1) && isfinite(pixel_offset),
                 "pram_tri_normalize: needs n_frames >= 0, n_rows >= 0 (0 without frames), a finite pixel_offset");
    const int rc = check_models(cam_model_host, n_frames, "pram_tri_normalize");
    if (rc != PRAM_OK) return rc;
    if (n_rows == 0) return PRAM_OK;
    hipLaunchKernelGGL(tri_normalize_kernel, dim3(cdiv(n_rows, 256)), dim3(256), 0, (hipStream_t)stream, keypoints, frame_off, cam_model,
                       cam_params, n_frames, n_rows, pixel_offset, norm);
    return pram_launch_status("pram_tri_normalize");
}

extern "C" int pram_tri_verify(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* matches,
                               const double* table, int n_frames, int n_pairs, int n_matches, double max_error, unsigned char* keep,
                               int* kept, int* edges, int* count, void* stream) {
    PRAM_REQUIRE(norm && frame_off && pairs && match_off && matches && table && keep && kept && edges && count, "pram_tri_verify: null pointer");
    PRAM_REQUIRE(aligned(norm, 8) && aligned(frame_off, 4) && aligned(pairs, 4) && aligned(match_off, 4) && aligned(matches, 4) &&
                 aligned(table, 8) && aligned(kept, 4) && aligned(edges, 4) && aligned(count, 4), "pram_tri_verify: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 0 && n_pairs >= 0 && n_matches >= 0 && max_error > 0.0,
                 "pram_tri_verify: needs n_frames >= 0, n_pairs >= 0, n_matches >= 0, max_error > 0");
    if (n_pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(tri_verify_kernel, dim3(n_pairs), dim3(256), 0, (hipStream_t)stream, norm, frame_off, pairs, match_off, matches, table,
                       n_frames, n_matches, max_error, keep, kept, edges, count);
    return pram_launch_status("pram_tri_verify");
}

extern "C" int pram_tri_components(const int* edges, int n_edges, int n_rows, int first_round, int n_rounds, int* label, int* state,
                                   void* stream) {
    PRAM_REQUIRE(edges && label && state, "pram_tri_components: null pointer");
    PRAM_REQUIRE(aligned(edges, 4) && aligned(label, 4) && aligned(state, 4), "pram_tri_components: misaligned pointer");
    PRAM_REQUIRE(n_edges >= 0 && n_rows >= 0 && n_rows <= MAX_ROWS && first_round >= 0 && n_rounds >= 0 && n_rounds <= 1024,
                 "pram_tri_components: needs n_edges >= 0, 0 <= n_rows <= 2^30, first_round >= 0, 0 <= n_rounds <= 1024");
    hipStream_t st = (hipStream_t)stream;
    if (first_round == 0) hipLaunchKernelGGL(tri_cc_init_kernel, dim3(cdiv(n_rows > 0 ? n_rows : 1, 256)), dim3(256), 0, st, label, n_rows, state);
    for (int r = 0; r < n_rounds; ++r) {
        if (n_edges) hipLaunchKernelGGL(tri_cc_hook_kernel, dim3(cdiv(n_edges, 256)), dim3(256), 0, st, edges, n_edges, n_rows, label, state);
        if (n_rows) hipLaunchKernelGGL(tri_cc_jump_kernel, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, label, n_rows, state);
        hipLaunchKernelGGL(tri_cc_end_kernel, dim3(1), dim3(1), 0, st, state);
    }
    return pram_launch_status("pram_tri_components");
}

extern "C" size_t pram_tri_tracks_workspace_bytes(int n_rows) {
    if (n_rows < 0 || n_rows > MAX_ROWS) return 0;
    return carve_scan_ws(nullptr, n_rows, 2 * track_blocks(n_rows), 2 * row_stride(n_rows), nullptr);      // rest: the two sums' local offsets
}

extern "C" int pram_tri_tracks(const int* label, const int* frame_off, int n_frames, int n_rows, void* workspace, size_t workspace_bytes,
                               int* trk_off, int* trk_label, int* trk_row, int* trk_frame, int* trk_kpt, int* sizes, void* stream) {
    PRAM_REQUIRE(label && frame_off && workspace && trk_off && trk_label && trk_row && trk_frame && trk_kpt && sizes, "pram_tri_tracks: null pointer");
    PRAM_REQUIRE(aligned(label, 4) && aligned(frame_off, 4) && aligned(workspace, 256) && aligned(trk_off, 4) && aligned(trk_label, 4) &&
                 aligned(trk_row, 4) && aligned(trk_frame, 4) && aligned(trk_kpt, 4) && aligned(sizes, 4), "pram_tri_tracks: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 0 && n_rows >= 0 && n_rows <= MAX_ROWS && (n_rows == 0 || n_frames >= 1),
                 "pram_tri_tracks: needs n_frames >= 0, 0 <= n_rows <= 2^30 (0 without frames)");
    PRAM_REQUIRE(workspace_bytes >= pram_tri_tracks_workspace_bytes(n_rows), "pram_tri_tracks: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const size_t stride = row_stride(n_rows);
    const int nb = track_blocks(n_rows);
    ScanWs ws;
    carve_scan_ws(workspace, n_rows, 2 * nb, 2 * stride, &ws);
    const TrackScan u = {{ws.rest, ws.rest + stride / sizeof(int)}, sizes, trk_off};
    if (hipMemsetAsync(ws.count, 0, 2 * stride, st) != hipSuccess) return pram_launch_status("pram_tri_tracks");      // count and cursor
    if (n_rows) hipLaunchKernelGGL(tri_count_kernel, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, label, n_rows, ws.count);
    hipLaunchKernelGGL(tri_scan_blocks_kernel<TrackScan>, dim3(nb), dim3(SCAN), 0, st, ws.count, n_rows, n_rows, u, ws.bsum);
    hipLaunchKernelGGL(tri_scan_totals_kernel<TrackScan>, dim3(1), dim3(256), 0, st, ws.bsum, nb, u);
    if (n_rows >= 2) {
        hipLaunchKernelGGL(tri_fill_kernel, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, label, ws, u, n_rows, trk_label, trk_row);
        hipLaunchKernelGGL(tri_sort_kernel, dim3(n_rows / 2), dim3(64), 0, st, sizes, trk_off, trk_row, n_rows);
        hipLaunchKernelGGL(tri_derive_kernel, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, sizes, trk_row, frame_off, n_frames, n_rows, trk_frame,
                           trk_kpt);
    }
    return pram_launch_status("pram_tri_tracks");
}

extern "C" int pram_tri_triangulate(const double* norm, const float* keypoints, const double* table, const int* cam_model,
                                    const double* cam_params, const int* trk_off, const int* trk_label, const int* trk_row,
                                    const int* trk_frame, int n_tracks, int n_entries, int n_frames, int n_rows, int trials,
                                    unsigned long long seed, double min_tri_angle, double max_reproj_error, int* accept, double* xyz,
                                    double* error, int* kept, int* best, unsigned char* entry_keep, double* entry_error, void* stream) {
    PRAM_REQUIRE(norm && keypoints && table && cam_model && cam_params && trk_off && trk_label && trk_row && trk_frame && accept && xyz && error &&
                 kept && best && entry_keep && entry_error, "pram_tri_triangulate: null pointer");
    PRAM_REQUIRE(aligned(norm, 8) && aligned(keypoints, 4) && aligned(table, 8) && aligned(cam_model, 4) && aligned(cam_params, 8) &&
                 aligned(trk_off, 4) && aligned(trk_label, 4) && aligned(trk_row, 4) && aligned(trk_frame, 4) && aligned(accept, 4) &&
                 aligned(xyz, 8) && aligned(error, 8) && aligned(kept, 4) && aligned(best, 4) && aligned(entry_error, 8),
                 "pram_tri_triangulate: misaligned pointer");
    PRAM_REQUIRE(n_tracks >= 0 && n_entries >= 0 && n_frames >= 0 && n_rows >= 0 && trials >= 1 && trials <= (1 << 24) && min_tri_angle >= 0.0 &&
                 max_reproj_error > 0.0,
                 "pram_tri_triangulate: needs n_tracks >= 0, n_entries >= 0, n_frames >= 0, n_rows >= 0, 1 <= trials <= 2^24, min_tri_angle >= 0, max_reproj_error > 0");
    if (n_tracks == 0) return PRAM_OK;
    const Obs g = {norm, keypoints, table, cam_model, cam_params, n_frames, n_rows};
    hipLaunchKernelGGL(tri_triangulate_kernel, dim3(n_tracks), dim3(64), 0, (hipStream_t)stream, g, trk_off, trk_label, trk_row, trk_frame,
                       n_entries, trials, seed, min_tri_angle, max_reproj_error, accept, xyz, error, kept, best, entry_keep, entry_error);
    return pram_launch_status("pram_tri_triangulate");
}

extern "C" size_t pram_tri_adjacency_workspace_bytes(int n_rows, int n_edges) {
    if (n_rows < 0 || n_rows > MAX_ROWS || n_edges < 0 || n_edges >= MAX_ROWS) return 0;
    return carve_scan_ws(nullptr, n_rows, adj_blocks(n_rows), align_up(sizeof(int)), nullptr);      // rest: the sort's number of lists
}

extern "C" int pram_tri_adjacency(const int* edges, int n_edges, const int* frame_off, int n_frames, int n_rows, void* workspace,
                                  size_t workspace_bytes, int* adj_off, int* adj, int* row_frame, void* stream) {
    PRAM_REQUIRE(edges && frame_off && workspace && adj_off && adj && row_frame, "pram_tri_adjacency: null pointer");
    PRAM_REQUIRE(aligned(edges, 4) && aligned(frame_off, 4) && aligned(workspace, 256) && aligned(adj_off, 4) && aligned(adj, 4) &&
                 aligned(row_frame, 4), "pram_tri_adjacency: misaligned pointer");
    PRAM_REQUIRE(n_edges >= 0 && n_edges < MAX_ROWS && n_frames >= 0 && n_rows >= 0 && n_rows <= MAX_ROWS && (n_rows == 0 || n_frames >= 1),
                 "pram_tri_adjacency: needs 0 <= n_edges < 2^30, n_frames >= 0, 0 <= n_rows <= 2^30 (0 without frames)");
    PRAM_REQUIRE(workspace_bytes >= pram_tri_adjacency_workspace_bytes(n_rows, n_edges), "pram_tri_adjacency: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nb = adj_blocks(n_rows);
    ScanWs ws;
    carve_scan_ws(workspace, n_rows, nb, align_up(sizeof(int)), &ws);
    const AdjScan u = {{adj_off}, ws.rest, n_rows};
    if (hipMemsetAsync(ws.count, 0, 2 * row_stride(n_rows), st) != hipSuccess) return pram_launch_status("pram_tri_adjacency");      // count and cursor
    if (n_edges && n_rows) hipLaunchKernelGGL(tri_adj_count_kernel, dim3(cdiv(n_edges, 256)), dim3(256), 0, st, edges, n_edges, n_rows, ws.count);
    hipLaunchKernelGGL(tri_scan_blocks_kernel<AdjScan>, dim3(nb), dim3(SCAN), 0, st, ws.count, n_rows, n_rows + 1, u, ws.bsum);
    hipLaunchKernelGGL(tri_scan_totals_kernel<AdjScan>, dim3(1), dim3(256), 0, st, ws.bsum, nb, u);
    hipLaunchKernelGGL(tri_adj_offsets_kernel, dim3(cdiv(n_rows + 1, 256)), dim3(256), 0, st, ws, frame_off, n_frames, n_rows, adj_off, row_frame);
    if (n_edges && n_rows) {
        hipLaunchKernelGGL(tri_adj_fill_kernel, dim3(cdiv(n_edges, 256)), dim3(256), 0, st, edges, n_edges, n_rows, ws, adj_off, adj);
        hipLaunchKernelGGL(tri_sort_kernel, dim3(n_rows), dim3(64), 0, st, u.segments, adj_off, adj, 2 * n_edges);
    }
    return pram_launch_status("pram_tri_adjacency");
}

extern "C" int pram_tri_support(const double* norm, const float* keypoints, const double* table, const int* cam_model,
                                const double* cam_params, const int* edges, int n_edges, const int* adj_off, const int* adj,
                                const int* row_frame, int n_frames, int n_rows, double min_tri_angle, double max_reproj_error,
                                int min_support, int* support, int* edges_out, void* stream) {
    PRAM_REQUIRE(norm && keypoints && table && cam_model && cam_params && edges && adj_off && adj && row_frame && support && edges_out,
                 "pram_tri_support: null pointer");
    PRAM_REQUIRE(aligned(norm, 8) && aligned(keypoints, 4) && aligned(table, 8) && aligned(cam_model, 4) && aligned(cam_params, 8) &&
                 aligned(edges, 4) && aligned(adj_off, 4) && aligned(adj, 4) && aligned(row_frame, 4) && aligned(support, 4) &&
                 aligned(edges_out, 4), "pram_tri_support: misaligned pointer");
    PRAM_REQUIRE(n_edges >= 0 && n_edges < MAX_ROWS && n_frames >= 0 && n_rows >= 0 && n_rows <= MAX_ROWS && min_support >= 0 &&
                 min_tri_angle >= 0.0 && max_reproj_error > 0.0,
                 "pram_tri_support: needs 0 <= n_edges < 2^30, n_frames >= 0, 0 <= n_rows <= 2^30, min_support >= 0, min_tri_angle >= 0, max_reproj_error > 0");
    if (n_edges == 0) return PRAM_OK;
    const Obs g = {norm, keypoints, table, cam_model, cam_params, n_frames, n_rows};
    const Adj a = {adj_off, adj, row_frame, 2 * n_edges};
    hipLaunchKernelGGL(tri_support_kernel, dim3(cdiv(n_edges, SUP_WAVES)), dim3(64 * SUP_WAVES), 0, (hipStream_t)stream, g, a, edges, n_edges,
                       min_tri_angle, max_reproj_error, min_support, support, edges_out);
    return pram_launch_status("pram_tri_support");
}

extern "C" int pram_tri_split(const int* trk_off, const int* trk_row, int n_tracks, int n_entries, const int* accept,
                              const unsigned char* entry_keep, const int* edges, int n_edges, int n_rows, int first, unsigned char* state,
                              int* edges_out, int* n_live, void* stream) {
    PRAM_REQUIRE(trk_off && trk_row && accept && entry_keep && edges && state && edges_out && n_live, "pram_tri_split: null pointer");
    PRAM_REQUIRE(aligned(trk_off, 4) && aligned(trk_row, 4) && aligned(accept, 4) && aligned(edges, 4) && aligned(edges_out, 4) &&
                 aligned(n_live, 4), "pram_tri_split: misaligned pointer");
    PRAM_REQUIRE(n_tracks >= 0 && n_entries >= 0 && n_entries <= MAX_ROWS && n_edges >= 0 && n_edges < MAX_ROWS && n_rows >= 0 && n_rows <= MAX_ROWS &&
                 (first == 0 || first == 1),
                 "pram_tri_split: needs n_tracks >= 0, 0 <= n_entries <= 2^30, 0 <= n_edges < 2^30, 0 <= n_rows <= 2^30, first 0 or 1");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tri_split_init_kernel, dim3(cdiv(first && n_rows > 0 ? n_rows : 1, 256)), dim3(256), 0, st, state, n_rows, first, n_live);
    if (n_tracks && n_entries && n_rows)
        hipLaunchKernelGGL(tri_split_mark_kernel, dim3(cdiv(n_entries, 256)), dim3(256), 0, st, trk_off, trk_row, n_tracks, n_entries, accept,
                           entry_keep, n_rows, state);
    if (n_edges)
        hipLaunchKernelGGL(tri_split_filter_kernel, dim3(cdiv(n_edges, 256)), dim3(256), 0, st, edges, n_edges, n_rows, state, edges_out, n_live);
    return pram_launch_status("pram_tri_split");
}
