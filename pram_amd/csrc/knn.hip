// Statistical outlier removal of a map's points: what RecMap.remove_statics_outlier of the reference (recognition/recmap.py:43-61)
// takes from Open3D's RemoveStatisticalOutliers, as include/pram_hip.h states it (not pinned to Open3D: DESIGN.md 4.22).
//   * pram_knn_mean_distance: every point's mean distance to its kk nearest points, itself included.  All pairs, exact: one
//     thread per query, the candidates through LDS as three float64 planes (every lane reads the same word: a broadcast), the
//     query's smallest d2 as a sorted list in registers.
//   * pram_sor_select: the valid points' mean and sample deviation in the k-means order of sums (blocks of PRAM_SOR_BLOCK, a block
//     added serially by one thread, the block sums in block order by one workgroup), then the mask and an ordered compaction of
//     the inliers' indices on workgroup.h's chunk_offset.
// Float64 throughout, every product and sum written out (the library is built with -ffp-contract=off); no floating-point atomics;
// plain stores only; no workgroup waits for another; every loop is bounded by an argument.
#include "glue.h"

namespace {

constexpr int TILE = PRAM_KNN_TILE, KMAX = PRAM_KNN_MAX_K, SB = PRAM_SOR_BLOCK;
constexpr int QB = 256;      // queries per workgroup, and the threads of every kernel here
static_assert(TILE % QB == 0 && TILE % 4 == 0, "a tile is loaded in whole passes of the workgroup and read four candidates at a time");
static_assert(SB % QB == 0, "a block of the sums is a whole number of 256-point chunks");

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double neg_inf() { return __longlong_as_double((long long)0xfff0000000000000ULL); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// d into the ascending list l, whose largest entry falls out: every slot takes the median of (its lower neighbour, itself, d).
// The slots are independent of one another (each reads the old values: the walk goes down), the indices are compile-time
// constants, so the list stays in registers.  A slot that holds -inf keeps it and passes nothing down.
template <int KS>
__device__ __forceinline__ void list_insert(double (&l)[KS], double d) {
#pragma unroll
    for (int j = KS - 1; j > 0; --j) {
        const double lo = l[j - 1], hi = l[j];
        l[j] = d < lo ? lo : (d < hi ? d : hi);
    }
    l[0] = d < l[0] ? d : l[0];
}

// ---------------------------------------------------------------------------------------------------------------- k nearest
// KS list slots, of which the last kk are in use: the first KS - kk hold -inf, which no candidate displaces, so the worst kept
// value is always l[KS - 1] and the list needs no runtime index.  A candidate is compared with l[KS - 1] first; once the list is
// warm almost every one fails, and the insertion is off the common path.  Padded candidates of the last tile carry +inf in every
// plane: their d2 is +inf, which is never < anything (the test is strict), so the tile is read four candidates at a time with no
// bound inside.  A padded query computes like the others (it takes part in the barriers) and writes nothing.
template <int KS>
__global__ __launch_bounds__(QB) void knn_mean_distance_kernel(const double* __restrict__ x, int n, int kk, double* __restrict__ avg) {
    __shared__ double sc[3][TILE];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * QB + tid;
    const bool on = i < n;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    if (on) { q0 = x[i * 3]; q1 = x[i * 3 + 1]; q2 = x[i * 3 + 2]; }
    const int start = KS - kk;
    double l[KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) l[j] = j < start ? neg_inf() : pos_inf();
    for (long long c0 = 0; c0 < n; c0 += TILE) {
        const int m = n - c0 < TILE ? (int)(n - c0) : TILE;
        const int m4 = (m + 3) & ~3;
        __syncthreads();      // the previous tile's readers
        for (int j = tid; j < m4; j += QB) {
            const bool in = j < m;
            sc[0][j] = in ? x[(c0 + j) * 3] : pos_inf();
            sc[1][j] = in ? x[(c0 + j) * 3 + 1] : pos_inf();
            sc[2][j] = in ? x[(c0 + j) * 3 + 2] : pos_inf();
        }
        __syncthreads();
        for (int j = 0; j < m4; j += 4) {
            double d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double a = sc[0][j + u] - q0, b = sc[1][j + u] - q1, c = sc[2][j + u] - q2;
                d[u] = (a * a + b * b) + c * c;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (d[u] < l[KS - 1]) list_insert<KS>(l, d[u]);      // strict; a NaN d2 fails it
        }
    }
    if (!on) return;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < KS; ++j)
        if (j >= start) s += sqrt(l[j]);      // ascending
    avg[i] = s / (double)kk;
}

// ---------------------------------------------------------------------------------------------------------------- the two sums
// PASS 1: the valid points' avg and their number per block; PASS 2: their squared deviations from stats[0].  The block through
// LDS, thread 0 adds it in index order; an invalid point adds nothing.
template <int PASS>
__global__ __launch_bounds__(QB) void sor_block_sums_kernel(const double* __restrict__ avg, int n, const double* __restrict__ stats,
                                                            double* __restrict__ part, int* __restrict__ vcnt) {
    __shared__ double sv[SB];
    const int tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * SB;
    const int m = n - i0 < SB ? (int)(n - i0) : SB;
    for (int j = tid; j < m; j += QB) sv[j] = avg[i0 + j];
    __syncthreads();
    if (tid == 0) {
        const double mean = PASS == 2 ? stats[0] : 0.0;
        double a = 0.0;
        int c = 0;
#pragma unroll 8
        for (int j = 0; j < m; ++j) {
            const double v = sv[j];
            if (v > 0.0) {
                const double d = v - mean;
                a += PASS == 2 ? d * d : v;
                ++c;
            }
        }
        part[blockIdx.x] = a;
        if (PASS == 1) vcnt[blockIdx.x] = c;
    }
}

// One workgroup: the block sums in block order.  PASS 1: mean and nv; PASS 2: std and threshold (NaN with nv < 2).
template <int PASS>
__global__ __launch_bounds__(QB) void sor_finish_kernel(const double* __restrict__ part, const int* __restrict__ vcnt, int nb, double std_ratio,
                                                        double* __restrict__ stats, int* __restrict__ count) {
    __shared__ double sv[SB];
    __shared__ int si[SB];
    const int tid = threadIdx.x;
    double a = 0.0;
    long long c = 0;
    for (int b0 = 0; b0 < nb; b0 += SB) {
        const int m = nb - b0 < SB ? nb - b0 : SB;
        __syncthreads();
        for (int j = tid; j < m; j += QB) {
            sv[j] = part[b0 + j];
            if (PASS == 1) si[j] = vcnt[b0 + j];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll 8
            for (int j = 0; j < m; ++j) {
                a += sv[j];
                if (PASS == 1) c += si[j];
            }
        }
    }
    if (tid != 0) return;
    if (PASS == 1) {
        const int nv = c > 0x7fffffffLL ? 0x7fffffff : (int)c;
        stats[0] = a / (double)nv;
        stats[3] = (double)nv;
        count[1] = nv;
    } else {
        const int nv = count[1];
        const double sd = nv >= 2 ? sqrt(a / (double)(nv - 1)) : quiet_nan();
        stats[1] = sd;
        stats[2] = nv >= 2 ? stats[0] + std_ratio * sd : quiet_nan();
    }
}

// ---------------------------------------------------------------------------------------------------------------- selection
__device__ __forceinline__ bool sor_inlier(double v, double threshold) { return v > 0.0 && v < threshold; }      // a NaN threshold keeps nothing

// the inliers of every block of SB points: icnt [nb]
__global__ __launch_bounds__(QB) void sor_count_kernel(const double* __restrict__ avg, int n, const double* __restrict__ stats, int* __restrict__ icnt) {
    __shared__ int wsum[QB / 64];
    const int tid = threadIdx.x;
    const double th = stats[2];
    int base = 0;
    for (int sub = 0; sub < SB / QB; ++sub) {
        const long long i = (long long)blockIdx.x * SB + sub * QB + tid;
        int total;
        chunk_offset<QB / 64>(i < n && sor_inlier(avg[i < n ? i : 0], th), wsum, total);
        base += total;
    }
    if (tid == 0) icnt[blockIdx.x] = base;
}

// One workgroup: ibase [nb], the exclusive running sum of icnt, and the number of inliers.
__global__ __launch_bounds__(QB) void sor_scan_kernel(const int* __restrict__ icnt, int nb, int* __restrict__ ibase, int* __restrict__ count) {
    __shared__ int wsum[QB / 64];
    const int tid = threadIdx.x;
    int base = 0;
    for (int b0 = 0; b0 < nb; b0 += QB) {
        const int b = b0 + tid;
        const int c = b < nb ? icnt[b] : 0;
        int total;
        const int o = chunk_offset_n<QB / 64>(c, wsum, total);
        if (b < nb) ibase[b] = base + o;
        base += total;
    }
    if (tid == 0) count[0] = base;
}

// the mask, and every inlier's index at its block's base plus its place inside the block
__global__ __launch_bounds__(QB) void sor_write_kernel(const double* __restrict__ avg, int n, const double* __restrict__ stats,
                                                       const int* __restrict__ ibase, unsigned char* __restrict__ mask, int* __restrict__ inlier_idx) {
    __shared__ int wsum[QB / 64];
    const int tid = threadIdx.x;
    const double th = stats[2];
    long long base = ibase[blockIdx.x];
    for (int sub = 0; sub < SB / QB; ++sub) {
        const long long i = (long long)blockIdx.x * SB + sub * QB + tid;
        const bool f = i < n && sor_inlier(avg[i < n ? i : 0], th);
        int total;
        const int o = chunk_offset<QB / 64>(f, wsum, total);
        if (i < n) mask[i] = f ? 1 : 0;
        if (f && base + o >= 0 && base + o < n) inlier_idx[base + o] = (int)i;
        base += total;
    }
}

static bool n_ok(long long n) { return n >= 1 && n < (1LL << 31); }

struct Layout { size_t part, vcnt, icnt, ibase, bytes; };      // part: doubles from the start; the others: ints from the end of part

static Layout layout(long long n) {
    const size_t nb = (size_t)((n + SB - 1) / SB);
    Layout L;
    L.part = 0;
    L.vcnt = 0; L.icnt = nb; L.ibase = 2 * nb;
    L.bytes = 8 * nb + 4 * 3 * nb;
    return L;
}

template <int KS>
static void launch_knn(const double* x, long long n, int kk, double* avg, hipStream_t s) {
    hipLaunchKernelGGL(knn_mean_distance_kernel<KS>, dim3((unsigned)((n + QB - 1) / QB)), dim3(QB), 0, s, x, (int)n, kk, avg);
}

}  // namespace

extern "C" int pram_knn_mean_distance(const double* x, long long n, int k, double* avg, void* stream) {
    PRAM_REQUIRE(x && avg, "pram_knn_mean_distance: null pointer");
    PRAM_REQUIRE(aligned(x, 8) && aligned(avg, 8), "pram_knn_mean_distance: float64 buffers must be 8-byte aligned");
    PRAM_REQUIRE(n_ok(n), "pram_knn_mean_distance: needs 1 <= n < 2^31, got n = %lld", n);
    PRAM_REQUIRE(k >= 1 && k <= KMAX, "pram_knn_mean_distance: needs 1 <= k <= PRAM_KNN_MAX_K = %d, got k = %d", KMAX, k);
    const int kk = k < n ? k : (int)n;
    hipStream_t s = (hipStream_t)stream;
    // the smallest list that holds kk: an insertion costs one step per slot
    if (kk <= 8) launch_knn<8>(x, n, kk, avg, s);
    else if (kk <= 16) launch_knn<16>(x, n, kk, avg, s);
    else if (kk <= 24) launch_knn<24>(x, n, kk, avg, s);
    else launch_knn<KMAX>(x, n, kk, avg, s);
    return pram_launch_status("pram_knn_mean_distance");
}

extern "C" size_t pram_sor_workspace_bytes(long long n) { return n_ok(n) ? layout(n).bytes : 0; }

extern "C" int pram_sor_select(const double* avg, long long n, double std_ratio, void* workspace, size_t workspace_bytes, double* stats,
                               unsigned char* mask, int* inlier_idx, int* count, void* stream) {
    PRAM_REQUIRE(avg && workspace && stats && mask && inlier_idx && count, "pram_sor_select: null pointer");
    PRAM_REQUIRE(aligned(avg, 8) && aligned(workspace, 8) && aligned(stats, 8), "pram_sor_select: float64 buffers and the workspace must be 8-byte aligned");
    PRAM_REQUIRE(aligned(inlier_idx, 4) && aligned(count, 4), "pram_sor_select: misaligned pointer");
    PRAM_REQUIRE(n_ok(n), "pram_sor_select: needs 1 <= n < 2^31, got n = %lld", n);
    PRAM_REQUIRE(std_ratio > 0.0, "pram_sor_select: needs std_ratio > 0, got %g", std_ratio);
    const Layout L = layout(n);
    PRAM_REQUIRE(workspace_bytes >= L.bytes, "pram_sor_select: workspace of %zu bytes, needs %zu (pram_sor_workspace_bytes)", workspace_bytes, L.bytes);
    const int N = (int)n, nb = (int)((n + SB - 1) / SB);
    double* part = static_cast<double*>(workspace) + L.part;
    int* wi = reinterpret_cast<int*>(static_cast<double*>(workspace) + nb);
    int *vcnt = wi + L.vcnt, *icnt = wi + L.icnt, *ibase = wi + L.ibase;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sor_block_sums_kernel<1>, dim3(nb), dim3(QB), 0, s, avg, N, (const double*)stats, part, vcnt);
    hipLaunchKernelGGL(sor_finish_kernel<1>, dim3(1), dim3(QB), 0, s, (const double*)part, (const int*)vcnt, nb, std_ratio, stats, count);
    hipLaunchKernelGGL(sor_block_sums_kernel<2>, dim3(nb), dim3(QB), 0, s, avg, N, (const double*)stats, part, vcnt);
    hipLaunchKernelGGL(sor_finish_kernel<2>, dim3(1), dim3(QB), 0, s, (const double*)part, (const int*)vcnt, nb, std_ratio, stats, count);
    hipLaunchKernelGGL(sor_count_kernel, dim3(nb), dim3(QB), 0, s, avg, N, (const double*)stats, icnt);
    hipLaunchKernelGGL(sor_scan_kernel, dim3(1), dim3(QB), 0, s, (const int*)icnt, nb, ibase, count);
    hipLaunchKernelGGL(sor_write_kernel, dim3(nb), dim3(QB), 0, s, avg, N, (const double*)stats, (const int*)ibase, mask, inlier_idx);
    return pram_launch_status("pram_sor_select");
}
