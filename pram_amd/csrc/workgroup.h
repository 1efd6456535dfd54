// The collectives of a wave and of a workgroup, once, for every file that adds, compares or compacts across lanes: the float64
// geometry (camera.h and through it ransac.h, obs.h, pose.hip, twoview.hip, bundle.hip, triangulate.hip) and the glue and map
// kernels (glue.h and through it mapper.hip, mapbuild.hip, compress.hip, retrieval.hip, knn.hip, kmeans.hip and the localisation
// glue).  The order of a sum is part of what the library promises: it is written down here and nowhere else.
// Everything with a barrier is called by every thread of the workgroup, from uniform control flow, and says what its barriers are for.
#pragma once
#include "common.h"

// ---------------------------------------------------------------- one wave: butterflies over the 64 lanes (lane l with l ^ 32, then
// ^ 16, 8, 4, 2, 1: both partners combine the same two values, so every lane ends with the same result, bit for bit)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the same from ^ 16 on: the sum of each half wave (32 lanes) in its lanes
__device__ __forceinline__ double half_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {      // fmax: a NaN loses to a number
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

// the smallest m of the wave and the smallest i among the lanes that hold it (a comparison with a NaN is false: no exchange)
__device__ __forceinline__ void wave_argmin_f64(double& m, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (om < m || (om == m && oi < i)) { m = om; i = oi; }
    }
}

// ---------------------------------------------------------------- a workgroup of WAVES waves
// The sum of v over the workgroup, to every thread: the waves' sums added in ascending wave order.  Two barriers: the first lets
// the previous call's readers of wsum [WAVES] finish, the second publishes this call's sums.  Both also order whatever the
// workgroup wrote before the call against what it reads after it.
template <int WAVES>
__device__ __forceinline__ int block_sum_i32(int v, int* wsum) {
    v = wave_sum_i32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    v = wsum[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += wsum[w];
    return v;
}

// The largest key of the workgroup, to every thread.  Two barriers with the contract of block_sum_i32, on wbest [WAVES].
template <int WAVES>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* wbest) {
    v = wave_max_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = v;
    __syncthreads();
    v = wbest[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v = wbest[w] > v ? wbest[w] : v;
    return v;
}

// The fixed-order fold of NV doubles per thread over a workgroup of 4 waves (256 threads, NV <= 256): the butterfly of
// wave_sum_f64 per value, then tot[e] = ((w0 + w1) + w2) + w3 over the waves' sums.  Every thread may read tot [NV] after the
// call.  Three barriers: the first lets the previous call's readers of wred / tot finish (ba_frames, ba_mv_frames and ba_cost of
// bundle.hip call it once per workgroup and had none: the one instruction the shared form adds to them), the second publishes
// wred [4][NV], the third tot.
template <int NV>
__device__ __forceinline__ void block_fold_f64(const double* acc, double (*wred)[NV], double* tot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const double s = wave_sum_f64(acc[e]);
        if (lane == 0) wred[wave][e] = s;
    }
    __syncthreads();
    if (tid < NV) tot[tid] = ((wred[0][tid] + wred[1][tid]) + wred[2][tid]) + wred[3][tid];
    __syncthreads();
}

// Ordered compaction inside a workgroup of WAVES waves, one chunk of 64 * WAVES items per call; every thread of the workgroup
// calls it.  Returns the offset of this thread's items among the chunk's (thread order) and the chunk's total through `total`;
// the caller adds the running base, a register every thread carries.  Two barriers: the first lets the previous call's readers
// of wsum [WAVES] finish, the second publishes this call's sums.
// Flag form: one item or none per thread.
template <int WAVES>
__device__ __forceinline__ int chunk_offset(bool f, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { if (w < wave) woff += wsum[w]; tot += wsum[w]; }
    total = tot;
    return woff + before;
}

// Count form: n >= 0 items per thread.  A caller that compacts in place (reads a chunk, calls this, writes at or before the
// positions read so far: phase 2 of projref_project_kernel) relies on a barrier standing between the chunk's reads and its
// writes; both barriers here do.
template <int WAVES>
__device__ __forceinline__ int chunk_offset_n(int n, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { if (w < wave) woff += wsum[w]; tot += wsum[w]; }
    total = tot;
    return woff + incl - n;
}
