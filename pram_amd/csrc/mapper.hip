// The glue of the incremental mapper (pram_amd/localization/mapper.py): what stands between the two-view stage,
// the absolute-pose stage, the triangulation and the bundle adjuster when a map grows from matches alone.  Seed scores per pair
// (the matches a relative pose triangulates in front of both cameras and the lower median of their angles), the seed choice, the
// 2D-3D correspondences of the frames that are not registered yet, the choice of the frames to try, their padded lists for
// pram_pose_*, and the edges between registered frames.  float64 wherever a coordinate is involved; counts are integers and every
// sum is an integer sum, so a result is a function of its inputs alone.  No workgroup waits for another.
#include "obs.h"
#include "glue.h"
#include <math.h>

namespace {

constexpr int LINKS = PRAM_MAP_MAX_LINKS;
constexpr int NO_POINT = 0x7fffffff;                 // an empty slot of a row's sorted list
constexpr unsigned long long NOT_COUNTED = ~0ull;    // the scratch word of a match that does not count: above every angle's bits

// ---------------------------------------------------------------- stage 1: the seed scores, one workgroup per pair
// Frame 0 is the world: its centre the origin, its rays as they are.  Frame 1 is (R, t) of the pair's qvec / tvec, laid out as a
// row of the frame table so that the rays, the midpoint and the depths are obs.h's.  The angles go to scratch as bit patterns;
// the lower median is the largest word w with fewer than k + 1 words below it, found bit by bit from the top: 64 counting passes.
__global__ __launch_bounds__(256) void map_pair_angles_kernel(const double* __restrict__ norm, const int* __restrict__ frame_off,
                                                              const int* __restrict__ pairs, const int* __restrict__ m_off,
                                                              const int* __restrict__ kept, const int* __restrict__ count,
                                                              const double* __restrict__ qvec, const double* __restrict__ tvec,
                                                              const int* __restrict__ success, int n_frames, int n_matches,
                                                              unsigned long long* scratch, int* __restrict__ n_tri,
                                                              double* __restrict__ tri_angle) {
    __shared__ int wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int f0 = pairs[(size_t)p * 2], f1 = pairs[(size_t)p * 2 + 1];
    int m0, m1;
    clamped_range(m_off[p], m_off[p + 1], n_matches, m0, m1);
    const int c = count[p];
    const int n = c < 0 ? 0 : (c > m1 - m0 ? m1 - m0 : c);      // the kept matches stand first in the pair's range
    const bool okp = success[p] != 0 && f0 >= 0 && f0 < n_frames && f1 >= 0 && f1 < n_frames;      // uniform
    int r0 = 0, r1 = 0, n0 = 0, n1 = 0;
    double T[FC];
#pragma unroll
    for (int a = 0; a < FC; ++a) T[a] = 0.0;
    if (okp) {
        r0 = frame_off[f0]; n0 = frame_off[f0 + 1] - r0;
        r1 = frame_off[f1]; n1 = frame_off[f1 + 1] - r1;
        const double* q = qvec + (size_t)p * 4;
        const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double qw = q[0] / nq, qx = q[1] / nq, qy = q[2] / nq, qz = q[3] / nq;
        const double tx = tvec[(size_t)p * 3], ty = tvec[(size_t)p * 3 + 1], tz = tvec[(size_t)p * 3 + 2];
        T[0] = 1.0 - 2.0 * qy * qy - 2.0 * qz * qz; T[1] = 2.0 * qx * qy - 2.0 * qw * qz; T[2] = 2.0 * qz * qx + 2.0 * qw * qy;
        T[3] = 2.0 * qx * qy + 2.0 * qw * qz; T[4] = 1.0 - 2.0 * qx * qx - 2.0 * qz * qz; T[5] = 2.0 * qy * qz - 2.0 * qw * qx;
        T[6] = 2.0 * qz * qx - 2.0 * qw * qy; T[7] = 2.0 * qy * qz + 2.0 * qw * qx; T[8] = 1.0 - 2.0 * qx * qx - 2.0 * qy * qy;
        T[9] = tx; T[10] = ty; T[11] = tz;
        T[12] = -(T[0] * tx + T[3] * ty + T[6] * tz);
        T[13] = -(T[1] * tx + T[4] * ty + T[7] * tz);
        T[14] = -(T[2] * tx + T[5] * ty + T[8] * tz);
    }
    const V3 C0 = {0.0, 0.0, 0.0}, C1 = {T[12], T[13], T[14]};
    int mine = 0;
    for (int e = tid; e < n; e += 256) {
        const int i0 = kept[(size_t)(m0 + e) * 2], i1 = kept[(size_t)(m0 + e) * 2 + 1];
        unsigned long long word = NOT_COUNTED;
        if (okp && i0 >= 0 && i0 < n0 && i1 >= 0 && i1 < n1) {      // an index outside its frame is never dereferenced
            const double u0 = norm[(size_t)(r0 + i0) * 2], v0 = norm[(size_t)(r0 + i0) * 2 + 1];
            const double u1 = norm[(size_t)(r1 + i1) * 2], v1 = norm[(size_t)(r1 + i1) * 2 + 1];
            const double l0 = sqrt(u0 * u0 + v0 * v0 + 1.0), l1 = sqrt(u1 * u1 + v1 * v1 + 1.0);
            const V3 d0 = {u0 / l0, v0 / l0, 1.0 / l0};
            const double x = u1 / l1, y = v1 / l1, z = 1.0 / l1;
            const V3 d1 = {T[0] * x + T[3] * y + T[6] * z, T[1] * x + T[4] * y + T[7] * z, T[2] * x + T[5] * y + T[8] * z};
            const V3 X = ray_midpoint(C0, d0, C1, d1);
            const double z0 = X.z, z1 = T[6] * X.x + T[7] * X.y + T[8] * X.z + T[11];
            const double ang = angle(d0, d1);
            if (z0 > 0.0 && z1 > 0.0 && ang >= 0.0) word = (unsigned long long)__double_as_longlong(ang);      // NaN compares false
        }
        scratch[m0 + e] = word;
        mine += word != NOT_COUNTED;
    }
    const int total = block_sum_i32<4>(mine, wsum);      // its barriers also publish the workgroup's scratch words
    const int k = (total - 1) / 2;
    unsigned long long med = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = med | (1ull << bit);
        int below = 0;
        for (int e = tid; e < n; e += 256) below += scratch[m0 + e] < cand;
        if (block_sum_i32<4>(below, wsum) <= k) med = cand;
    }
    if (tid == 0) {
        n_tri[p] = total;
        tri_angle[p] = total > 0 ? __longlong_as_double((long long)med) : 0.0;
    }
}

// one workgroup: the eligible pair with the largest n_tri, the lowest position on a tie
__global__ __launch_bounds__(256) void map_seed_kernel(const int* __restrict__ success, const int* __restrict__ n_tri,
                                                       const double* __restrict__ tri_angle, int n_pairs, int min_num_inliers,
                                                       double min_tri_angle, int* __restrict__ seed) {
    __shared__ unsigned long long wbest[4];
    unsigned long long best = 0;
    for (int p = threadIdx.x; p < n_pairs; p += 256) {
        const int n = n_tri[p];
        const bool ok = success[p] != 0 && n >= min_num_inliers && tri_angle[p] >= min_tri_angle && n >= 0;
        const unsigned long long key = ((unsigned long long)(unsigned)n << 32) | (unsigned)(0x7fffffff - p);
        if (ok && key > best) best = key;
    }
    best = block_max_u64<4>(best, wbest);
    if (threadIdx.x == 0) seed[0] = best ? 0x7fffffff - (int)(best & 0xffffffffu) : -1;
}

// ---------------------------------------------------------------- stage 3: correspondences, one workgroup per frame
struct MapAdj { const int* off; const int* adj; const int* row_frame; int n; };

// The distinct points of row u's neighbours in registered frames, the LINKS smallest ascending in k (NO_POINT behind them);
// rest: the neighbours whose point is not among them.  Every index is checked before it is used.
__device__ __forceinline__ int row_links(const MapAdj& a, const unsigned char* __restrict__ registered, const int* __restrict__ row_point,
                                         int n_frames, int n_rows, int n_points, int u, int* k, int& rest) {
#pragma unroll
    for (int i = 0; i < LINKS; ++i) k[i] = NO_POINT;
    int beg, end;
    clamped_range(a.off[u], a.off[u + 1], a.n, beg, end);
    const auto point_of = [&](int e) -> int {
        const int v = a.adj[e];
        if (v < 0 || v >= n_rows) return -1;
        const int fv = a.row_frame[v];
        if (fv < 0 || fv >= n_frames || registered[fv] == 0) return -1;
        const int pt = row_point[v];
        return pt >= 0 && pt < n_points ? pt : -1;
    };
    for (int e = beg; e < end; ++e) {
        const int pt = point_of(e);
        if (pt < 0 || pt >= k[LINKS - 1]) continue;      // no point, the last slot's own, or beyond it
        bool dup = false;
#pragma unroll
        for (int i = 0; i < LINKS - 1; ++i) dup = dup || k[i] == pt;
        if (dup) continue;
#pragma unroll
        for (int i = LINKS - 1; i >= 1; --i) k[i] = pt < k[i - 1] ? k[i - 1] : (pt < k[i] ? pt : k[i]);
        k[0] = pt < k[0] ? pt : k[0];
    }
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < LINKS; ++i) cnt += k[i] != NO_POINT;
    rest = 0;
    if (cnt == LINKS)
        for (int e = beg; e < end; ++e) rest += point_of(e) > k[LINKS - 1];
    return cnt;
}

// FILL false: n_corr and dropped per frame.  FILL true: the rows, from corr_off[f] on, ordered by (row, point).
template <bool FILL>
__global__ __launch_bounds__(256) void map_correspond_kernel(MapAdj a, const int* __restrict__ frame_off,
                                                             const unsigned char* __restrict__ registered, const int* __restrict__ row_point,
                                                             int n_frames, int n_rows, int n_points, const int* __restrict__ corr_off, int cap,
                                                             int* __restrict__ n_corr, int* __restrict__ dropped, int* __restrict__ corr_row,
                                                             int* __restrict__ corr_point) {
    __shared__ int wsum[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    int beg = 0, end = 0;
    if (registered[f] == 0) clamped_range(frame_off[f], frame_off[f + 1], n_rows, beg, end);      // uniform; a registered frame has no row here
    int base = FILL ? corr_off[f] : 0, lost = 0;
    for (int c0 = beg; c0 < end; c0 += 256) {
        const int u = c0 + tid;
        int k[LINKS], cnt = 0, rest = 0;
        if (u < end) cnt = row_links(a, registered, row_point, n_frames, n_rows, n_points, u, k, rest);
        int total;
        const int o = chunk_offset_n<4>(cnt, wsum, total);
        if (FILL) {
#pragma unroll
            for (int i = 0; i < LINKS; ++i) {
                const long long at = (long long)base + o + i;
                if (i < cnt && at >= 0 && at < cap) { corr_row[at] = u; corr_point[at] = k[i]; }
            }
        }
        base += total;
        lost += rest;
    }
    if (!FILL) {
        lost = block_sum_i32<4>(lost, wsum);
        if (tid == 0) { n_corr[f] = base; dropped[f] = lost; }
    }
}

// one workgroup: corr_off [n_frames + 1], the exclusive sums of n_corr
__global__ __launch_bounds__(256) void map_offsets_kernel(const int* __restrict__ n_corr, int n_frames, int* __restrict__ corr_off) {
    __shared__ int wsum[4];
    int base = 0;
    for (int c0 = 0; c0 < n_frames; c0 += 256) {
        const int f = c0 + threadIdx.x;
        int total;
        const int o = chunk_offset_n<4>(f < n_frames ? n_corr[f] : 0, wsum, total);
        if (f < n_frames) corr_off[f] = base + o;
        base += total;
    }
    if (threadIdx.x == 0) corr_off[n_frames] = base;
}

// ---------------------------------------------------------------- stage 4: the frames to try and their padded lists
// one workgroup: selection rounds on (n_corr, then the smaller frame), each strictly after the round before
__global__ __launch_bounds__(256) void map_choose_kernel(const int* __restrict__ n_corr, const unsigned char* __restrict__ registered,
                                                         const int* __restrict__ tries, int n_frames, int min_corr, int max_reg_trials,
                                                         int rounds, int* __restrict__ chosen, int* __restrict__ chosen_count,
                                                         int* __restrict__ n_chosen) {
    __shared__ unsigned long long wbest[4];
    const int tid = threadIdx.x;
    for (int f = tid; f < n_frames; f += 256) { chosen[f] = -1; chosen_count[f] = 0; }
    unsigned long long prev = ~0ull;
    int found = 0;
    for (int r = 0; r < rounds; ++r) {
        unsigned long long best = 0;
        for (int f = tid; f < n_frames; f += 256) {
            const int c = n_corr[f];
            const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)(0x7fffffff - f);
            if (registered[f] == 0 && c > 0 && c >= min_corr && tries[f] < max_reg_trials && key < prev && key > best) best = key;
        }
        best = block_max_u64<4>(best, wbest);
        if (best == 0) break;      // uniform: nothing left, every later round finds nothing either
        prev = best;
        if (tid == 0) { chosen[found] = 0x7fffffff - (int)(best & 0xffffffffu); chosen_count[found] = (int)(best >> 32); }
        ++found;
    }
    if (tid == 0) n_chosen[0] = found;
}

// grid (chosen frames, chunks of t0): the first min(n_corr, t0) rows of the frame's correspondences, zeros behind them
__global__ __launch_bounds__(256) void map_pack_kernel(const int* __restrict__ chosen, const int* __restrict__ corr_off,
                                                       const int* __restrict__ corr_row, const int* __restrict__ corr_point, int n_corr_total,
                                                       const float* __restrict__ keypoints, const double* __restrict__ xyz, int n_frames,
                                                       int n_rows, int n_points, int t0, float* __restrict__ m_kpts, double* __restrict__ m_xyz,
                                                       int* __restrict__ counts, int* __restrict__ cut) {
    const int s = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
    const int f = chosen[s];
    int beg = 0, end = 0;
    if (f >= 0 && f < n_frames) clamped_range(corr_off[f], corr_off[f + 1], n_corr_total, beg, end);
    const int n = end - beg, take = n < t0 ? n : t0;
    if (j == 0) { counts[s] = take; cut[s] = n - take; }
    if (j >= t0) return;
    float ku = 0.f, kv = 0.f;
    double x = 0.0, y = 0.0, z = 0.0;
    if (j < take) {
        const int r = corr_row[beg + j], pt = corr_point[beg + j];
        if (r >= 0 && r < n_rows && pt >= 0 && pt < n_points) {
            ku = keypoints[(size_t)r * 2]; kv = keypoints[(size_t)r * 2 + 1];
            x = xyz[(size_t)pt * 3]; y = xyz[(size_t)pt * 3 + 1]; z = xyz[(size_t)pt * 3 + 2];
        }
    }
    const size_t at = (size_t)s * t0 + j;
    m_kpts[at * 2] = ku; m_kpts[at * 2 + 1] = kv;
    m_xyz[at * 3] = x; m_xyz[at * 3 + 1] = y; m_xyz[at * 3 + 2] = z;
}

// ---------------------------------------------------------------- stage 5: the edges between registered frames
__global__ __launch_bounds__(256) void map_live_edges_kernel(const int* __restrict__ edges, int n_edges, const int* __restrict__ row_frame,
                                                             const unsigned char* __restrict__ registered, int n_frames, int n_rows,
                                                             int* __restrict__ edges_out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[(size_t)e * 2], v = edges[(size_t)e * 2 + 1];
    bool live = u >= 0 && v >= 0 && u < n_rows && v < n_rows;
    if (live) {
        const int fu = row_frame[u], fv = row_frame[v];
        live = fu >= 0 && fu < n_frames && fv >= 0 && fv < n_frames && registered[fu] != 0 && registered[fv] != 0;
    }
    edges_out[(size_t)e * 2] = live ? u : -1; edges_out[(size_t)e * 2 + 1] = live ? v : -1;
}

constexpr int MAX_ROWS = 1 << 30;

}  // namespace

extern "C" int pram_map_pair_angles(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* kept,
                                    const int* count, const double* qvec, const double* tvec, const int* success, int n_frames,
                                    int n_pairs, int n_matches, void* workspace, size_t workspace_bytes, int* n_tri, double* tri_angle,
                                    void* stream) {
    PRAM_REQUIRE(norm && frame_off && pairs && match_off && kept && count && qvec && tvec && success && workspace && n_tri && tri_angle,
                 "pram_map_pair_angles: null pointer");
    PRAM_REQUIRE(aligned(norm, 8) && aligned(frame_off, 4) && aligned(pairs, 4) && aligned(match_off, 4) && aligned(kept, 4) && aligned(count, 4) &&
                 aligned(qvec, 8) && aligned(tvec, 8) && aligned(success, 4) && aligned(workspace, 8) && aligned(n_tri, 4) && aligned(tri_angle, 8),
                 "pram_map_pair_angles: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 0 && n_pairs >= 0 && n_matches >= 0, "pram_map_pair_angles: needs n_frames >= 0, n_pairs >= 0, n_matches >= 0");
    PRAM_REQUIRE(workspace_bytes >= pram_map_pair_angles_workspace_bytes(n_matches), "pram_map_pair_angles: workspace too small");
    if (n_pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(map_pair_angles_kernel, dim3(n_pairs), dim3(256), 0, (hipStream_t)stream, norm, frame_off, pairs, match_off, kept, count,
                       qvec, tvec, success, n_frames, n_matches, static_cast<unsigned long long*>(workspace), n_tri, tri_angle);
    return pram_launch_status("pram_map_pair_angles");
}

extern "C" size_t pram_map_pair_angles_workspace_bytes(int n_matches) {
    return n_matches < 0 ? 0 : (size_t)(n_matches > 0 ? n_matches : 1) * sizeof(unsigned long long);
}

extern "C" int pram_map_seed(const int* success, const int* n_tri, const double* tri_angle, int n_pairs, int min_num_inliers,
                             double min_tri_angle, int* seed, void* stream) {
    PRAM_REQUIRE(success && n_tri && tri_angle && seed, "pram_map_seed: null pointer");
    PRAM_REQUIRE(aligned(success, 4) && aligned(n_tri, 4) && aligned(tri_angle, 8) && aligned(seed, 4), "pram_map_seed: misaligned pointer");
    PRAM_REQUIRE(n_pairs >= 0 && min_num_inliers >= 0 && min_tri_angle >= 0.0,
                 "pram_map_seed: needs n_pairs >= 0, min_num_inliers >= 0, min_tri_angle >= 0");
    hipLaunchKernelGGL(map_seed_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, success, n_tri, tri_angle, n_pairs, min_num_inliers,
                       min_tri_angle, seed);
    return pram_launch_status("pram_map_seed");
}

extern "C" int pram_map_correspond(const int* adj_off, const int* adj, const int* row_frame, int n_adj, const int* frame_off,
                                   const unsigned char* registered, const int* row_point, int n_frames, int n_rows, int n_points,
                                   int capacity, int* n_corr, int* corr_off, int* dropped, int* corr_row, int* corr_point, void* stream) {
    PRAM_REQUIRE(adj_off && adj && row_frame && frame_off && registered && row_point && n_corr && corr_off && dropped && corr_row && corr_point,
                 "pram_map_correspond: null pointer");
    PRAM_REQUIRE(aligned(adj_off, 4) && aligned(adj, 4) && aligned(row_frame, 4) && aligned(frame_off, 4) && aligned(row_point, 4) &&
                 aligned(n_corr, 4) && aligned(corr_off, 4) && aligned(dropped, 4) && aligned(corr_row, 4) && aligned(corr_point, 4),
                 "pram_map_correspond: misaligned pointer");
    PRAM_REQUIRE(n_adj >= 0 && n_frames >= 0 && n_rows >= 0 && n_rows <= MAX_ROWS / LINKS && n_points >= 0 && capacity >= 0 &&
                 (n_rows == 0 || n_frames >= 1),
                 "pram_map_correspond: needs n_adj >= 0, n_frames >= 0, 0 <= n_rows <= 2^27 (0 without frames), n_points >= 0, capacity >= 0");
    hipStream_t st = (hipStream_t)stream;
    const MapAdj a = {adj_off, adj, row_frame, n_adj};
    if (n_frames)
        hipLaunchKernelGGL(map_correspond_kernel<false>, dim3(n_frames), dim3(256), 0, st, a, frame_off, registered, row_point, n_frames, n_rows,
                           n_points, (const int*)nullptr, capacity, n_corr, dropped, corr_row, corr_point);
    hipLaunchKernelGGL(map_offsets_kernel, dim3(1), dim3(256), 0, st, n_corr, n_frames, corr_off);
    if (n_frames && capacity)
        hipLaunchKernelGGL(map_correspond_kernel<true>, dim3(n_frames), dim3(256), 0, st, a, frame_off, registered, row_point, n_frames, n_rows,
                           n_points, (const int*)corr_off, capacity, n_corr, dropped, corr_row, corr_point);
    return pram_launch_status("pram_map_correspond");
}

extern "C" int pram_map_choose(const int* n_corr, const unsigned char* registered, const int* tries, int n_frames, int min_corr,
                               int max_reg_trials, int round_frames, int* chosen, int* chosen_count, int* n_chosen, void* stream) {
    PRAM_REQUIRE(n_corr && registered && tries && chosen && chosen_count && n_chosen, "pram_map_choose: null pointer");
    PRAM_REQUIRE(aligned(n_corr, 4) && aligned(tries, 4) && aligned(chosen, 4) && aligned(chosen_count, 4) && aligned(n_chosen, 4),
                 "pram_map_choose: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 0 && min_corr >= 0 && max_reg_trials >= 0 && round_frames >= 0,
                 "pram_map_choose: needs n_frames >= 0, min_corr >= 0, max_reg_trials >= 0, round_frames >= 0");
    const int rounds = round_frames > 0 && round_frames < n_frames ? round_frames : n_frames;
    hipLaunchKernelGGL(map_choose_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_corr, registered, tries, n_frames, min_corr,
                       max_reg_trials, rounds, chosen, chosen_count, n_chosen);
    return pram_launch_status("pram_map_choose");
}

extern "C" int pram_map_pack(const int* chosen, int n_chosen, const int* corr_off, const int* corr_row, const int* corr_point,
                             int n_corr_total, const float* keypoints, const double* xyz, int n_frames, int n_rows, int n_points, int t0,
                             float* matched_keypoints, double* matched_xyzs, int* counts, int* cut, void* stream) {
    PRAM_REQUIRE(chosen && corr_off && corr_row && corr_point && keypoints && xyz && matched_keypoints && matched_xyzs && counts && cut,
                 "pram_map_pack: null pointer");
    PRAM_REQUIRE(aligned(chosen, 4) && aligned(corr_off, 4) && aligned(corr_row, 4) && aligned(corr_point, 4) && aligned(keypoints, 4) &&
                 aligned(xyz, 8) && aligned(matched_keypoints, 4) && aligned(matched_xyzs, 8) && aligned(counts, 4) && aligned(cut, 4),
                 "pram_map_pack: misaligned pointer");
    PRAM_REQUIRE(n_chosen >= 0 && n_chosen <= 65535 * 256 && n_corr_total >= 0 && n_frames >= 0 && n_rows >= 0 && n_points >= 0 && t0 >= 1 &&
                 t0 <= 65535 * 256,
                 "pram_map_pack: needs 0 <= n_chosen, n_corr_total >= 0, n_frames >= 0, n_rows >= 0, n_points >= 0, 1 <= t0 <= 65535 * 256");
    if (n_chosen == 0) return PRAM_OK;
    hipLaunchKernelGGL(map_pack_kernel, dim3(n_chosen, cdiv(t0, 256)), dim3(256), 0, (hipStream_t)stream, chosen, corr_off, corr_row, corr_point,
                       n_corr_total, keypoints, xyz, n_frames, n_rows, n_points, t0, matched_keypoints, matched_xyzs, counts, cut);
    return pram_launch_status("pram_map_pack");
}

extern "C" int pram_map_live_edges(const int* edges, int n_edges, const int* row_frame, const unsigned char* registered, int n_frames,
                                   int n_rows, int* edges_out, void* stream) {
    PRAM_REQUIRE(edges && row_frame && registered && edges_out, "pram_map_live_edges: null pointer");
    PRAM_REQUIRE(aligned(edges, 4) && aligned(row_frame, 4) && aligned(edges_out, 4), "pram_map_live_edges: misaligned pointer");
    PRAM_REQUIRE(n_edges >= 0 && n_edges < MAX_ROWS && n_frames >= 0 && n_rows >= 0 && n_rows <= MAX_ROWS,
                 "pram_map_live_edges: needs 0 <= n_edges < 2^30, n_frames >= 0, 0 <= n_rows <= 2^30");
    if (n_edges == 0) return PRAM_OK;
    hipLaunchKernelGGL(map_live_edges_kernel, dim3(cdiv(n_edges, 256)), dim3(256), 0, (hipStream_t)stream, edges, n_edges, row_frame, registered,
                       n_frames, n_rows, edges_out);
    return pram_launch_status("pram_map_live_edges");
}
