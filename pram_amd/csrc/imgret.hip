// Image retrieval: a VLAD vector per image from its 128-D local descriptors, and the top-k database images of
// every query by the inner product of two such vectors.  Four stages, each a function of its inputs alone:
//   assign     nearest centre per descriptor, float64 distance in a fixed order (one row per thread, the centres in LDS)
//   aggregate  per (image, centre) the sum of the residuals of the image's rows with that label, in ascending row index
//   normalize  intra-normalisation per centre block, then the global L2 norm, to float32
//   topk       exact-fp32 products on v_mfma_f32_32x32x2_f32, one accumulator chain per (query, database image) over the whole
//              length in ascending index, so that a value depends neither on the tile it falls in nor on the split; the best k per
//              query are kept as packed 64-bit keys (pram_covis_topk's trick); a second launch merges the splits' lists
// No floating-point atomics, no workgroup waits for another, every loop is bounded by an argument or a constant, nothing allocated.
#include "launch.h"
#include "workgroup.h"

namespace {

constexpr int D = PRAM_IMGRET_DIM;           // 128
constexpr int D4 = D / 4;

// ---------------------------------------------------------------- assign: 256 rows per workgroup, centres [k][128] in dynamic LDS
__global__ __launch_bounds__(256) void imgret_assign_kernel(const float* __restrict__ desc, const float* __restrict__ centres, int n_rows,
                                                            int k, int* __restrict__ labels, double* __restrict__ dist) {
    extern __shared__ float4 sc[];      // [k][32]
    const int tid = threadIdx.x;
    const float4* c4 = reinterpret_cast<const float4*>(centres);
    for (int i = tid; i < k * D4; i += 256) sc[i] = c4[i];
    const long long row = (long long)blockIdx.x * 256 + tid;
    const bool live = row < n_rows;
    const float4* x4 = reinterpret_cast<const float4*>(desc) + (size_t)(live ? row : n_rows - 1) * D4;
    float4 x[D4];      // the row stays in registers: every index below is a constant after unrolling
#pragma unroll
    for (int q = 0; q < D4; ++q) x[q] = x4[q];
    __syncthreads();
    double best = 0.0;
    int bi = 0;
    for (int c = 0; c < k; ++c) {
        const float4* cc = sc + c * D4;      // every lane reads the same address: a broadcast
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < D4; ++q) {
            const float4 cv = cc[q];
            const double d0 = (double)x[q].x - (double)cv.x, d1 = (double)x[q].y - (double)cv.y;
            const double d2 = (double)x[q].z - (double)cv.z, d3 = (double)x[q].w - (double)cv.w;
            s += d0 * d0; s += d1 * d1; s += d2 * d2; s += d3 * d3;
        }
        if (c == 0 || s < best) { best = s; bi = c; }      // strict: the lowest index wins a tie
    }
    if (live) { labels[row] = bi; dist[row] = best; }
}

// ---------------------------------------------------------------- aggregate: one workgroup of 128 threads per (image, centre),
// thread d; the image's labels go through LDS 128 at a time so that the walk over them does not wait for memory row by row
__global__ __launch_bounds__(128) void imgret_aggregate_kernel(const float* __restrict__ desc, const int* __restrict__ labels,
                                                               const float* __restrict__ centres, const int* __restrict__ first,
                                                               const int* __restrict__ count, int n_rows, int k,
                                                               double* __restrict__ sums, int* __restrict__ n_assigned) {
    __shared__ int lab[128];
    const int img = blockIdx.x, c = blockIdx.y, d = threadIdx.x;
    long long lo = first[img], hi = lo + (long long)count[img];      // clamped to the rows: nothing outside desc is read
    if (lo < 0) lo = 0;
    if (hi > n_rows) hi = n_rows;
    const double cd = (double)centres[(size_t)c * D + d];
    double acc = 0.0;
    int n = 0;
    for (long long r0 = lo; r0 < hi; r0 += 128) {
        const int len = (int)(hi - r0 < 128 ? hi - r0 : 128);
        __syncthreads();      // the previous chunk's readers are done
        lab[d] = d < len ? labels[r0 + d] : -1;
        __syncthreads();
        for (int j = 0; j < len; ++j) {
            if (lab[j] != c) continue;      // uniform over the workgroup
            acc += (double)desc[(size_t)(r0 + j) * D + d] - cd;
            ++n;
        }
    }
    sums[((size_t)img * k + c) * D + d] = acc;
    if (d == 0) n_assigned[(size_t)img * k + c] = n;
}

// ---------------------------------------------------------------- the vocabulary's Lloyd step: one thread per (centre, dimension)
// folds the blocks' partial sums in ascending block order onto the running total (the caller starts it at 0.0 and may hand the
// blocks over in several calls), then moves the centre
__global__ __launch_bounds__(256) void imgret_fold_kernel(const double* __restrict__ sums, const int* __restrict__ n_assigned, int n_blk,
                                                          int k, double* __restrict__ total, int* __restrict__ total_n) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // c * 128 + d
    if (i >= k * D) return;
    const int c = i / D;
    double acc = total[i];
    for (int b = 0; b < n_blk; ++b) acc += sums[(size_t)b * k * D + i];
    total[i] = acc;
    if (i - c * D == 0) {
        int n = total_n[c];
        for (int b = 0; b < n_blk; ++b) n += n_assigned[(size_t)b * k + c];
        total_n[c] = n;
    }
}

__global__ __launch_bounds__(256) void imgret_update_kernel(float* __restrict__ centres, const double* __restrict__ total,
                                                            const int* __restrict__ total_n, int k) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k * D) return;
    const int n = total_n[i / D];
    if (n > 0) centres[i] = (float)((double)centres[i] + total[i] / (double)n);      // a centre without a row keeps its value
}

// ---------------------------------------------------------------- normalize: one workgroup per image
constexpr int NORM_CHUNK = 2048;      // entries whose squares go through LDS per round of the global norm's chain

__global__ __launch_bounds__(256) void imgret_normalize_kernel(const double* __restrict__ sums, int k, float* __restrict__ out) {
    __shared__ double nrm[PRAM_IMGRET_MAX_K];
    __shared__ double sq[NORM_CHUNK];
    __shared__ double g_sh;
    const int img = blockIdx.x, tid = threadIdx.x;
    const double* v = sums + (size_t)img * k * D;
    const int total = k * D;
    // block norms: thread c walks its block in ascending d
    for (int c = tid; c < k; c += 256) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) { const double e = v[c * D + d]; s += e * e; }
        nrm[c] = sqrt(s);
    }
    __syncthreads();
    // the global norm: one chain over c ascending, d ascending; the squares are made by everybody, added by thread 0
    double g2 = 0.0;
    for (int i0 = 0; i0 < total; i0 += NORM_CHUNK) {      // total is a multiple of 128, NORM_CHUNK too
        const int len = total - i0 < NORM_CHUNK ? total - i0 : NORM_CHUNK;
        for (int i = tid; i < len; i += 256) {
            const double nc = nrm[(i0 + i) / D];
            const double e = nc > 0.0 ? v[i0 + i] / nc : 0.0;
            sq[i] = e * e;
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < len; ++i) g2 += sq[i];
        __syncthreads();
    }
    if (tid == 0) g_sh = sqrt(g2);
    __syncthreads();
    const double g = g_sh;
    for (int i = tid; i < total; i += 256) {
        const double nc = nrm[i / D];
        const double e = nc > 0.0 ? v[i] / nc : 0.0;
        out[(size_t)img * total + i] = g > 0.0 ? (float)(e / g) : 0.0f;
    }
}

// ---------------------------------------------------------------- top-k
// key: the float's bits made monotone (-0.0 first turned into +0.0), then 0x7fffffff - index: larger similarity first, then the
// smaller index.  0 is "nothing": no finite similarity gives it, and a NaN is turned into it.
__device__ __forceinline__ unsigned long long sim_key(float s, int idx) {
    if (s != s) return 0ull;
    unsigned b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0u;
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 32) | (unsigned)(0x7fffffff - idx);
}
__device__ __forceinline__ float key_sim(unsigned long long key) {
    unsigned b = (unsigned)(key >> 32);
    b = (b & 0x80000000u) ? (b & 0x7fffffffu) : ~b;
    return __uint_as_float(b);
}

constexpr int TK = PRAM_IMGRET_MAX_TOPK;      // 64: a list slot per lane
constexpr int QT = 32, DT = 128, BK = 32, LDT = BK + 4;      // query rows and database rows per tile, depth per LDS stage

// One wave merges NC * 64 candidates into its sorted list of 64 keys (both in LDS, the list descending, 0 = empty): every nonzero
// key is distinct, so its rank among all of them is its slot.  Only this wave touches `list` and `cand`; a wave's LDS accesses
// execute in program order, and the fences keep the compiler from moving them across the phases.
template <int NC>
__device__ __forceinline__ void wave_merge(unsigned long long* list, const unsigned long long* cand) {
    const int lane = threadIdx.x & 63;
    unsigned long long mine[NC + 1];
    mine[0] = list[lane];
#pragma unroll
    for (int i = 0; i < NC; ++i) mine[i + 1] = cand[i * 64 + lane];
    const unsigned long long thr = list[TK - 1];      // 0 while the list is not full
    bool any = false;
#pragma unroll
    for (int i = 0; i < NC; ++i) any = any || mine[i + 1] > thr;
    if (!__any(any)) return;      // wave-uniform
    int rank[NC + 1];
#pragma unroll
    for (int i = 0; i <= NC; ++i) rank[i] = 0;
    for (int j = 0; j < TK; ++j) {
        const unsigned long long o = list[j];
#pragma unroll
        for (int i = 0; i <= NC; ++i) rank[i] += o > mine[i];
    }
    for (int j = 0; j < NC * 64; ++j) {
        const unsigned long long o = cand[j];
#pragma unroll
        for (int i = 0; i <= NC; ++i) rank[i] += o > mine[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the slots below the number of nonzero keys are all written; the others were 0 before and stay 0
#pragma unroll
    for (int i = 0; i <= NC; ++i)
        if (mine[i] != 0ull && rank[i] < TK) list[rank[i]] = mine[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct alignas(16) TopkStage {
    float q[2][QT * LDT];
    float d[2][DT * LDT];
};      // 46,080 B
union TopkSmem {
    TopkStage st;
    unsigned long long cand[QT][DT];      // 32,768 B: the tile's keys, once its products are complete
};

// grid: (query tiles) x splits, 256 threads = 4 waves; wave w multiplies the 32 queries with database rows 32 w .. 32 w + 31 of the
// current 128-row tile, then merges the keys of queries 8 w .. 8 w + 7
__global__ __launch_bounds__(256) void imgret_topk_kernel(const float* __restrict__ q, int nq, const float* __restrict__ db, int nd, int L,
                                                          const int* __restrict__ exclude, const unsigned char* __restrict__ db_valid,
                                                          int k, int splits, int tiles_per_split, unsigned long long* __restrict__ partial) {
    __shared__ TopkSmem sm;
    __shared__ unsigned long long list[QT][TK];      // 16,384 B
    __shared__ int excl[QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x / splits, sp = blockIdx.x - qt * splits;
    const int q0 = qt * QT;
    const int r = lane & 31, h = lane >> 5;
    const int srow = tid >> 3, skq = tid & 7;      // staging: 8 float4 per row, 32 rows per pass
    // LDS image of a row: each group of 8 consecutive k is stored as k0 k2 k4 k6 | k1 k3 k5 k7, so that the lower half-wave's
    // b128 holds the even and the upper half-wave's the odd ones: MFMA step j then contracts k = 2j and 2j + 1, ascending
    const int swr = (skq >> 1) * 8 + (skq & 1) * 2;

    for (int i = tid; i < QT * TK; i += 256) (&list[0][0])[i] = 0ull;
    if (tid < QT) {
        const int qi = q0 + tid;
        excl[tid] = (exclude != nullptr && qi < nq) ? exclude[qi] : -1;
    }
    const int n_tiles = (nd + DT - 1) / DT;
    const int t_begin = sp * tiles_per_split;
    const int t_end = t_begin + tiles_per_split < n_tiles ? t_begin + tiles_per_split : n_tiles;
    const int nk = L / BK;
    // rows past the end are read from the last row (legal) and never reach a list
    const int qrow = q0 + srow < nq ? q0 + srow : nq - 1;
    const float4* qsrc = reinterpret_cast<const float4*>(q + (size_t)qrow * L) + skq;

    for (int t = t_begin; t < t_end; ++t) {
        const int d0 = t * DT;
        const float4* dsrc[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int row = d0 + srow + 32 * p;
            dsrc[p] = reinterpret_cast<const float4*>(db + (size_t)(row < nd ? row : nd - 1) * L) + skq;
        }
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        float4 rq, rd[4];
        auto issue = [&](int kt) {
            rq = qsrc[kt * (BK / 4)];
#pragma unroll
            for (int p = 0; p < 4; ++p) rd[p] = dsrc[p][kt * (BK / 4)];
        };
        auto commit = [&](int buf) {
            float* a = &sm.st.q[buf][srow * LDT + swr];
            *reinterpret_cast<float2*>(a) = make_float2(rq.x, rq.z);
            *reinterpret_cast<float2*>(a + 4) = make_float2(rq.y, rq.w);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float* b = &sm.st.d[buf][(srow + 32 * p) * LDT + swr];
                *reinterpret_cast<float2*>(b) = make_float2(rd[p].x, rd[p].z);
                *reinterpret_cast<float2*>(b + 4) = make_float2(rd[p].y, rd[p].w);
            }
        };
        __syncthreads();      // the previous tile's keys (the same LDS) have been merged
        issue(0);
        commit(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const bool more = kt + 1 < nk;
            if (more) issue(kt + 1);
            const float* sa = &sm.st.q[kt & 1][r * LDT + h * 4];
            const float* sb = &sm.st.d[kt & 1][(wave * 32 + r) * LDT + h * 4];
#pragma unroll
            for (int kk = 0; kk < BK / 8; ++kk) {
                const float4 a = *reinterpret_cast<const float4*>(sa + kk * 8);
                const float4 b = *reinterpret_cast<const float4*>(sb + kk * 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
            }
            if (more) commit((kt + 1) & 1);
            __syncthreads();
        }
        // the tile's keys: accumulator element e of this lane is query (e & 3) + 8 (e >> 2) + 4 h, database row d0 + 32 wave + r
        const int col = wave * 32 + r, j = d0 + col;
        const bool allowed = j < nd && (db_valid == nullptr || db_valid[j < nd ? j : 0] != 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int qi = (e & 3) + 8 * (e >> 2) + 4 * h;
            sm.cand[qi][col] = (allowed && excl[qi] != j) ? sim_key(acc[e], j) : 0ull;
        }
        __syncthreads();
        for (int i = 0; i < QT / 4; ++i) {
            const int qi = wave * (QT / 4) + i;
            wave_merge<DT / 64>(list[qi], sm.cand[qi]);
        }
    }
    __syncthreads();
    for (int i = tid; i < QT * k; i += 256) {
        const int qi = i / k, s = i - qi * k;
        if (q0 + qi < nq) partial[((size_t)(q0 + qi) * splits + sp) * k + s] = list[qi][s];
    }
}

// one wave per query: the splits' lists merged one after the other, then unpacked
__global__ __launch_bounds__(64) void imgret_topk_merge_kernel(const unsigned long long* __restrict__ partial, int splits, int k,
                                                               int* __restrict__ idx, float* __restrict__ sim) {
    __shared__ unsigned long long list[TK];
    __shared__ unsigned long long cand[64];
    const int qi = blockIdx.x, lane = threadIdx.x;
    list[lane] = 0ull;
    for (int s = 0; s < splits; ++s) {
        cand[lane] = lane < k ? partial[((size_t)qi * splits + s) * k + lane] : 0ull;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        wave_merge<1>(list, cand);
    }
    if (lane < k) {
        const unsigned long long key = list[lane];
        idx[(size_t)qi * k + lane] = key ? 0x7fffffff - (int)(key & 0xffffffffu) : -1;
        sim[(size_t)qi * k + lane] = key ? key_sim(key) : 0.0f;
    }
}

}  // namespace

extern "C" int pram_imgret_assign(const float* desc, int n_rows, const float* centres, int k, int* labels, double* dist, void* stream) {
    PRAM_REQUIRE(desc && centres && labels && dist, "pram_imgret_assign: null pointer");
    PRAM_REQUIRE(aligned(desc, 16) && aligned(centres, 16) && aligned(labels, 4) && aligned(dist, 8),
                 "pram_imgret_assign: misaligned pointer (rows 16 bytes, float64 8)");
    PRAM_REQUIRE(k >= 1 && k <= PRAM_IMGRET_MAX_K, "pram_imgret_assign: needs 1 <= k <= %d, got %d", PRAM_IMGRET_MAX_K, k);
    PRAM_REQUIRE(n_rows >= 0, "pram_imgret_assign: needs n_rows >= 0");
    if (n_rows == 0) return PRAM_OK;
    opt_in_lds<imgret_assign_kernel>((size_t)PRAM_IMGRET_MAX_K * D * sizeof(float));
    hipLaunchKernelGGL(imgret_assign_kernel, dim3(cdiv(n_rows, 256)), dim3(256), (size_t)k * D * sizeof(float), (hipStream_t)stream, desc, centres,
                       n_rows, k, labels, dist);
    return pram_launch_status("pram_imgret_assign");
}

extern "C" int pram_imgret_aggregate(const float* desc, const int* labels, int n_rows, const float* centres, int k, const int* first,
                                     const int* count, int n_img, double* sums, int* n_assigned, void* stream) {
    PRAM_REQUIRE(desc && labels && centres && first && count && sums && n_assigned, "pram_imgret_aggregate: null pointer");
    PRAM_REQUIRE(aligned(desc, 4) && aligned(labels, 4) && aligned(centres, 4) && aligned(first, 4) && aligned(count, 4) && aligned(sums, 8) &&
                 aligned(n_assigned, 4), "pram_imgret_aggregate: misaligned pointer (float64 8 bytes)");
    PRAM_REQUIRE(k >= 1 && k <= PRAM_IMGRET_MAX_K, "pram_imgret_aggregate: needs 1 <= k <= %d, got %d", PRAM_IMGRET_MAX_K, k);
    PRAM_REQUIRE(n_rows >= 0 && n_img >= 0, "pram_imgret_aggregate: needs n_rows >= 0 and n_img >= 0");
    if (n_img == 0) return PRAM_OK;
    hipLaunchKernelGGL(imgret_aggregate_kernel, dim3(n_img, k), dim3(128), 0, (hipStream_t)stream, desc, labels, centres, first, count, n_rows,
                       k, sums, n_assigned);
    return pram_launch_status("pram_imgret_aggregate");
}

extern "C" int pram_imgret_fold(const double* sums, const int* n_assigned, int n_blk, int k, double* total, int* total_n, void* stream) {
    PRAM_REQUIRE(sums && n_assigned && total && total_n, "pram_imgret_fold: null pointer");
    PRAM_REQUIRE(aligned(sums, 8) && aligned(total, 8) && aligned(n_assigned, 4) && aligned(total_n, 4),
                 "pram_imgret_fold: misaligned pointer (float64 8 bytes)");
    PRAM_REQUIRE(k >= 1 && k <= PRAM_IMGRET_MAX_K, "pram_imgret_fold: needs 1 <= k <= %d, got %d", PRAM_IMGRET_MAX_K, k);
    PRAM_REQUIRE(n_blk >= 0, "pram_imgret_fold: needs n_blk >= 0");
    if (n_blk == 0) return PRAM_OK;
    hipLaunchKernelGGL(imgret_fold_kernel, dim3(cdiv(k * D, 256)), dim3(256), 0, (hipStream_t)stream, sums, n_assigned, n_blk, k, total, total_n);
    return pram_launch_status("pram_imgret_fold");
}

extern "C" int pram_imgret_update(float* centres, const double* total, const int* total_n, int k, void* stream) {
    PRAM_REQUIRE(centres && total && total_n, "pram_imgret_update: null pointer");
    PRAM_REQUIRE(aligned(centres, 4) && aligned(total, 8) && aligned(total_n, 4), "pram_imgret_update: misaligned pointer (float64 8 bytes)");
    PRAM_REQUIRE(k >= 1 && k <= PRAM_IMGRET_MAX_K, "pram_imgret_update: needs 1 <= k <= %d, got %d", PRAM_IMGRET_MAX_K, k);
    hipLaunchKernelGGL(imgret_update_kernel, dim3(cdiv(k * D, 256)), dim3(256), 0, (hipStream_t)stream, centres, total, total_n, k);
    return pram_launch_status("pram_imgret_update");
}

extern "C" int pram_imgret_normalize(const double* sums, int n_img, int k, float* out, void* stream) {
    PRAM_REQUIRE(sums && out, "pram_imgret_normalize: null pointer");
    PRAM_REQUIRE(aligned(sums, 8) && aligned(out, 4), "pram_imgret_normalize: misaligned pointer (float64 8 bytes)");
    PRAM_REQUIRE(k >= 1 && k <= PRAM_IMGRET_MAX_K, "pram_imgret_normalize: needs 1 <= k <= %d, got %d", PRAM_IMGRET_MAX_K, k);
    PRAM_REQUIRE(n_img >= 0, "pram_imgret_normalize: needs n_img >= 0");
    if (n_img == 0) return PRAM_OK;
    hipLaunchKernelGGL(imgret_normalize_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, sums, k, out);
    return pram_launch_status("pram_imgret_normalize");
}

extern "C" size_t pram_imgret_topk_workspace_bytes(int nq, int k, int splits) {
    if (nq < 0 || k < 1 || k > PRAM_IMGRET_MAX_TOPK || splits < 1 || splits > PRAM_IMGRET_MAX_SPLITS) return 0;
    return (size_t)(nq > 0 ? nq : 1) * splits * k * sizeof(unsigned long long);
}

extern "C" int pram_imgret_topk(const float* q, int nq, const float* db, int nd, int L, const int* exclude, const unsigned char* db_valid,
                                int k, int splits, void* workspace, size_t workspace_bytes, int* idx, float* sim, void* stream) {
    PRAM_REQUIRE(q && db && workspace && idx && sim, "pram_imgret_topk: null pointer");
    PRAM_REQUIRE(aligned(q, 16) && aligned(db, 16) && aligned(exclude, 4) && aligned(workspace, 8) && aligned(idx, 4) && aligned(sim, 4),
                 "pram_imgret_topk: misaligned pointer (rows 16 bytes, workspace 8)");
    PRAM_REQUIRE(k >= 1 && k <= PRAM_IMGRET_MAX_TOPK, "pram_imgret_topk: needs 1 <= k <= %d, got %d", PRAM_IMGRET_MAX_TOPK, k);
    PRAM_REQUIRE(L >= D && L % D == 0, "pram_imgret_topk: L must be a positive multiple of %d, got %d", D, L);
    PRAM_REQUIRE(nd >= 1, "pram_imgret_topk: needs nd >= 1");
    PRAM_REQUIRE(nq >= 0, "pram_imgret_topk: needs nq >= 0");
    PRAM_REQUIRE(splits >= 1 && splits <= PRAM_IMGRET_MAX_SPLITS, "pram_imgret_topk: needs 1 <= splits <= %d, got %d", PRAM_IMGRET_MAX_SPLITS, splits);
    PRAM_REQUIRE((long long)cdiv(nq, QT) * splits < 2147483647LL, "pram_imgret_topk: query tiles * splits overflow the grid");
    PRAM_REQUIRE(workspace_bytes >= pram_imgret_topk_workspace_bytes(nq, k, splits), "pram_imgret_topk: workspace too small (%zu < %zu bytes)",
                 workspace_bytes, pram_imgret_topk_workspace_bytes(nq, k, splits));
    if (nq == 0) return PRAM_OK;
    const int n_tiles = cdiv(nd, DT);
    hipLaunchKernelGGL(imgret_topk_kernel, dim3(cdiv(nq, QT) * splits), dim3(256), 0, (hipStream_t)stream, q, nq, db, nd, L, exclude, db_valid, k,
                       splits, cdiv(n_tiles, splits), (unsigned long long*)workspace);
    if (pram_launch_status("pram_imgret_topk") != PRAM_OK) return PRAM_E_LAUNCH;
    hipLaunchKernelGGL(imgret_topk_merge_kernel, dim3(nq), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)workspace, splits, k, idx,
                       sim);
    return pram_launch_status("pram_imgret_topk");
}
