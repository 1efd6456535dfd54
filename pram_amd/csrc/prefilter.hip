// The query pre-filter of Frame.add_segmentations (localization/frame.py:96-121) for a padded batch: a frame whose recogniser
// leaves enough non-background keypoints keeps only those, in their order, before the vote, the matcher and the tracker see it.
// The softmax, the mask and its count are pram_seg_epilogue_f32's; nothing here recomputes them.  Two kernels: a plan (one
// workgroup per query: the decision, the ordered compaction of the row indices by ballot and prefix, the counts) and a row mover
// (one wave per OUTPUT row, the descriptor row as 16-byte vectors).  Bandwidth kernels: plain vector loads and stores, no atomics,
// nothing allocated, no host synchronisation.
#include "glue.h"

namespace {

// frame.py:106: torch.sum(non_bg_mask) >= 0.4 * n, the right side in float64.  The integer form 5 * k >= 2 * n is the same test
// for every n an int holds: fl(0.4) = 0.4 (1 + d) with d < 2^-53, so for a multiple of 5 the product fl(0.4) * n lies within
// half an ulp of the integer 2 n / 5 and rounds to it, and for any other n the exact 2 n / 5 has a fractional part of at least
// 0.2, which a relative error of 2^-52 cannot carry across an integer below 2^31.
__device__ __forceinline__ bool prefilter_fires(int enable, int n_non_bg, int n) {
    return enable != 0 && 5LL * (long long)n_non_bg >= 2LL * (long long)n;
}

// one workgroup per query: kept [b][j] = the input row of output row j (-1 for j >= o_counts[b]), o_counts, filtered
__global__ __launch_bounds__(256) void prefilter_plan_kernel(const int* __restrict__ non_bg, const int* __restrict__ n_non_bg,
                                                             const int* __restrict__ counts, int enable, int n, int* __restrict__ kept,
                                                             int* __restrict__ o_counts, int* __restrict__ filtered) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int cnt = counts[b];
    cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    const bool fires = prefilter_fires(enable, n_non_bg[b], cnt);      // uniform over the workgroup
    const int* mask = non_bg + (size_t)b * n;
    int* row = kept + (size_t)b * n;
    int base = 0;      // a running sum every thread carries
    for (int c0 = 0; c0 < cnt; c0 += 256) {
        const int i = c0 + tid;
        const bool f = i < cnt && (!fires || mask[i] != 0);
        int tot;
        const int o = base + chunk_offset<4>(f, wsum, tot);
        if (f) row[o] = i;      // o <= i < n
        base += tot;
    }
    for (int j = base + tid; j < n; j += 256) row[j] = -1;
    if (tid == 0) { o_counts[b] = base; filtered[b] = fires ? 1 : 0; }
}

// one wave per output row; grid cdiv(n, 4) * batch.  A kept row is moved as 32-bit words (so NaN payloads and negative zeros
// survive), the descriptor row as 16-byte vectors; a logits row starts at a 4-byte boundary only (n_class is odd in every
// shipped configuration), so it moves as words, 256 contiguous bytes per wave instruction.  A row beyond the count is zero,
// its seg id -2 (pram_seg_epilogue_f32's fill).
__global__ __launch_bounds__(256) void prefilter_rows_kernel(const unsigned* __restrict__ kpts, const unsigned* __restrict__ scores,
                                                             const f32x4* __restrict__ desc, const unsigned* __restrict__ logits,
                                                             const int* __restrict__ seg_ids, const int* __restrict__ kept, int n, int c,
                                                             int d4, int blocks_per_query, unsigned* __restrict__ o_kpts,
                                                             unsigned* __restrict__ o_scores, f32x4* __restrict__ o_desc,
                                                             unsigned* __restrict__ o_logits, int* __restrict__ o_seg_ids) {
    const int b = blockIdx.x / blocks_per_query, lane = threadIdx.x & 63;
    const int j = (blockIdx.x - b * blocks_per_query) * 4 + (threadIdx.x >> 6);
    if (j >= n) return;      // wave-uniform
    const size_t dst = (size_t)b * n + j;
    int s = kept[dst];
    if (s >= n) s = -1;
    const bool live = s >= 0;      // wave-uniform
    const size_t src = (size_t)b * n + (size_t)(live ? s : 0);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int v = lane; v < d4; v += 64) o_desc[dst * d4 + v] = live ? desc[src * d4 + v] : zero4;
    for (int k = lane; k < c; k += 64) o_logits[dst * c + k] = live ? logits[src * c + k] : 0u;
    if (lane < 2) o_kpts[dst * 2 + lane] = live ? kpts[src * 2 + lane] : 0u;
    else if (lane == 2) o_scores[dst] = live ? scores[src] : 0u;
    else if (lane == 3) o_seg_ids[dst] = live ? seg_ids[src] : -2;
}

}  // namespace

extern "C" int pram_query_prefilter(const float* keypoints, const float* scores, const float* descriptors, const float* logits,
                                    const int* seg_ids, const int* non_bg_mask, const int* n_non_bg, const int* counts, int enable,
                                    int batch, int n, int n_class, int desc_dim, float* o_keypoints, float* o_scores,
                                    float* o_descriptors, float* o_logits, int* o_seg_ids, int* o_counts, int* kept, int* filtered,
                                    void* stream) {
    PRAM_REQUIRE(keypoints && scores && descriptors && logits && seg_ids && non_bg_mask && n_non_bg && counts && o_keypoints && o_scores &&
                 o_descriptors && o_logits && o_seg_ids && o_counts && kept && filtered, "pram_query_prefilter: null pointer");
    PRAM_REQUIRE(batch >= 0 && n >= 0 && n_class >= 1, "pram_query_prefilter: needs batch >= 0, n >= 0, n_class >= 1");
    PRAM_REQUIRE(desc_dim >= 0 && desc_dim % 4 == 0, "pram_query_prefilter: desc_dim must be a multiple of 4 (16-byte descriptor rows)");
    PRAM_REQUIRE(aligned(descriptors, 16) && aligned(o_descriptors, 16), "pram_query_prefilter: descriptors must be 16-byte aligned");
    PRAM_REQUIRE(aligned(keypoints, 4) && aligned(scores, 4) && aligned(logits, 4) && aligned(seg_ids, 4) && aligned(non_bg_mask, 4) &&
                 aligned(n_non_bg, 4) && aligned(counts, 4) && aligned(o_keypoints, 4) && aligned(o_scores, 4) && aligned(o_logits, 4) &&
                 aligned(o_seg_ids, 4) && aligned(o_counts, 4) && aligned(kept, 4) && aligned(filtered, 4), "pram_query_prefilter: misaligned pointer");
    PRAM_REQUIRE(keypoints != o_keypoints && scores != o_scores && descriptors != o_descriptors && logits != o_logits && seg_ids != o_seg_ids,
                 "pram_query_prefilter: the outputs must not be the inputs");
    PRAM_REQUIRE((long long)batch * cdiv(n, 4) < 2147483647LL, "pram_query_prefilter: batch * n / 4 does not fit the launch grid");
    if (batch == 0 || n == 0) return PRAM_OK;
    hipLaunchKernelGGL(prefilter_plan_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, non_bg_mask, n_non_bg, counts, enable, n, kept,
                       o_counts, filtered);
    const int bpq = cdiv(n, 4);
    hipLaunchKernelGGL(prefilter_rows_kernel, dim3(batch * bpq), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned*>(keypoints),
                       reinterpret_cast<const unsigned*>(scores), reinterpret_cast<const f32x4*>(descriptors),
                       reinterpret_cast<const unsigned*>(logits), seg_ids, kept, n, n_class, desc_dim / 4, bpq,
                       reinterpret_cast<unsigned*>(o_keypoints), reinterpret_cast<unsigned*>(o_scores), reinterpret_cast<f32x4*>(o_descriptors),
                       reinterpret_cast<unsigned*>(o_logits), o_seg_ids);
    return pram_launch_status("pram_query_prefilter");
}
