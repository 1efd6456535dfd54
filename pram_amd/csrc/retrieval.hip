// Localisation against retrieved database frames (localization/pose_estimator.py: feature_matching :45-86, find_2D_3D_matches
// :89-134, pose_estimator_hloc :138-270, pose_refinement :273-376, pose_estimator_iterative :380-612, get_covisibility_frames
// :18-42): the glue around the grouped matcher call.  A (query, retrieved frame) pair is a plan row of the candidate stage ("all
// keypoints of the query" against "the frame's rows that carry a 3D point"), so pram_cand_gather / pram_cand_correspond run on the
// plan written here unchanged, handed valid_rows in place of sel_rows, and pram_refine_merge stacks a query's slots.  Latency /
// bandwidth kernels: plain vector loads and stores, integer atomics only (the results do not depend on the order the adds arrive
// in), every loop bounded by an argument, nothing allocated.
#include "glue.h"

namespace {

// one thread per (query b, slot j < n_db)
__global__ __launch_bounds__(256) void retr_plan_kernel(const int* __restrict__ retrieval, const int* __restrict__ counts,
                                                        const int* __restrict__ enable, const int* __restrict__ frame_off,
                                                        const int* __restrict__ valid_off, int batch, int n_db, int n_frames,
                                                        int n_valid, int* __restrict__ plan) {
    const int p = blockIdx.x * 256 + threadIdx.x, pairs = batch * n_db;
    if (p >= pairs) return;
    const int b = p / n_db, j = p - b * n_db;
    int g = retrieval[p];
    if (g < 0 || g >= n_frames) g = -1;
    const int nq = counts[b];
    int v0 = 0, nv = 0;
    if (g >= 0) clamped_range(valid_off[g], valid_off[g + 1], n_valid, v0, nv);
    nv -= v0;
    // feature_matching :65-66: a frame without a row that carries a point answers all -1
    const bool live = g >= 0 && nv > 0 && nq > 0 && (enable == nullptr || enable[b] != 0);
    int* col = plan + p;      // column-major table: field X of pair p at plan[X * pairs + p]
    col[PL_QUERY * pairs] = b; col[PL_SID * pairs] = -1; col[PL_FRAME * pairs] = live ? g : -1; col[PL_SEM * pairs] = 0;
    col[PL_LEN0 * pairs] = live ? nq : 0;
    col[PL_LEN1 * pairs] = live ? nv : 0;
    col[PL_TOK_OFF * pairs] = -1; col[PL_ROW0 * pairs] = live ? frame_off[g] : 0; col[PL_SEL_OFF * pairs] = live ? v0 : -1;
    col[PL_ORDER * pairs] = j;
}

// observations of point `id`: the length of its frame list, 0 for an id the table does not hold
__device__ __forceinline__ int observation_count(const long long* __restrict__ pt_ids, const int* __restrict__ pt_off, int n_points, long long id) {
    const int lo = lower_bound_i64(pt_ids, n_points, id);
    if (lo >= n_points || pt_ids[lo] != id) return 0;
    return pt_off[lo + 1] - pt_off[lo];
}

// one workgroup per pair: ordered compaction of the rows whose point has obs_th observations or more (:122)
__global__ __launch_bounds__(256) void retr_filter_kernel(ConstMatchList r, const int* __restrict__ r_count, int t0,
                                                          const long long* __restrict__ pt_ids, const int* __restrict__ pt_off,
                                                          int n_points, int obs_th, MatchList m, int* __restrict__ m_count) {
    __shared__ int wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    int n = r_count[p];
    n = n < 0 ? 0 : (n > t0 ? t0 : n);
    int base = 0;      // a running sum every thread carries
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        const size_t q = (size_t)p * t0 + i;
        const bool f = i < n && (obs_th <= 0 || observation_count(pt_ids, pt_off, n_points, r.p3d[q]) >= obs_th);
        int tot;
        const int o = base + chunk_offset<4>(f, wsum, tot);
        if (f) match_copy_row(m, (size_t)p * t0 + o, r, q);
        base += tot;
    }
    if (tid == 0) m_count[p] = base;
}

// one thread per query: the walk of pose_estimator_iterative over its slots (:429-556, then :558)
__global__ __launch_bounds__(256) void retr_select_kernel(const int* __restrict__ success, const int* __restrict__ num_inliers,
                                                          const int* __restrict__ count, int batch, int n_db, int inlier_th,
                                                          int min_best_inliers, int* __restrict__ chosen) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    int best = -1, best_inl = 0, kept = -1;      // :414 best_results['num_inliers'] starts at 0: a slot needs more to become best
    for (int j = 0; j < n_db; ++j) {
        const size_t p = (size_t)b * n_db + j;
        if (count[p] < 8 || success[p] == 0) continue;      // :440, :465
        const int inl = num_inliers[p];
        if (inl > best_inl) { best = j; best_inl = inl; }      // :481
        if (inl >= inlier_th) { kept = j; break; }             // :491
    }
    int status = 1;
    if (kept < 0) {
        const bool take = best >= 0 && best_inl >= min_best_inliers;      // :558
        kept = take ? best : -1;
        status = take ? 2 : 0;
    }
    chosen[b * 3] = kept; chosen[b * 3 + 1] = status; chosen[b * 3 + 2] = best;
}

// one workgroup per listed frame: the counts into hist [n][n_frames] (global memory, zeroed by the entry), then k selection rounds
__global__ __launch_bounds__(256) void covis_topk_kernel(const int* __restrict__ frames, const int* __restrict__ valid_off,
                                                         const int* __restrict__ valid_rows, const long long* __restrict__ point3d_ids,
                                                         int n_rows, int n_valid, const long long* __restrict__ pt_ids,
                                                         const int* __restrict__ pt_off, const int* __restrict__ pt_frames, int n_points,
                                                         int n_entries, int n_frames, int k, int include_self, int* hist,
                                                         int* __restrict__ best_frames, int* __restrict__ best_counts,
                                                         int* __restrict__ n_found) {
    __shared__ unsigned long long wbest[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    int f = frames[s];
    if (f < 0 || f >= n_frames) f = -1;      // a frame the store does not hold shares nothing with anyone
    int v0 = 0, v1 = 0;
    if (f >= 0) clamped_range(valid_off[f], valid_off[f + 1], n_valid, v0, v1);
    int* h = hist + (size_t)s * n_frames;
    for (int v = v0 + tid; v < v1; v += 256) {
        const int row = valid_rows[v];
        if (row < 0 || row >= n_rows) continue;
        const long long id = point3d_ids[row];
        const int lo = lower_bound_i64(pt_ids, n_points, id);
        if (lo >= n_points || pt_ids[lo] != id) continue;
        int e0, e1;
        clamped_range(pt_off[lo], pt_off[lo + 1], n_entries, e0, e1);
        for (int e = e0; e < e1; ++e) {
            const int g = pt_frames[e];
            if (g >= 0 && g < n_frames && (include_self || g != f)) atomicAdd(&h[g], 1);      // :25
        }
    }
    __threadfence();
    __syncthreads();
    // round r takes the largest (count, then smaller frame index) strictly after round r - 1's pick; the counts are read past this
    // compute unit's vector cache, which may hold a line of a neighbouring frame's histogram from before the adds
    unsigned long long prev = ~0ull;
    int found = 0;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = 0;
        for (int g = tid; g < n_frames; g += 256) {
            const int c = __hip_atomic_load(&h[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)(0x7fffffff - g);
            if (c > 0 && key < prev && key > best) best = key;
        }
        best = block_max_u64<4>(best, wbest);
        if (best != 0) { prev = best; ++found; }
        else prev = 0;      // nothing left: every later round finds nothing either
        if (tid == 0) {
            best_frames[(size_t)s * k + r] = best ? 0x7fffffff - (int)(best & 0xffffffffu) : -1;
            best_counts[(size_t)s * k + r] = (int)(best >> 32);
        }
    }
    if (tid == 0) n_found[s] = found;
}

}  // namespace

extern "C" int pram_retr_plan(const int* retrieval, const int* counts, const int* enable, const int* frame_off, const int* valid_off,
                              int batch, int n_db, int n_frames, int n_valid, int* plan, void* stream) {
    PRAM_REQUIRE(retrieval && counts && frame_off && valid_off && plan, "pram_retr_plan: null pointer");
    PRAM_REQUIRE(aligned(retrieval, 4) && aligned(counts, 4) && aligned(enable, 4) && aligned(frame_off, 4) && aligned(valid_off, 4) &&
                 aligned(plan, 4), "pram_retr_plan: misaligned pointer");
    PRAM_REQUIRE(n_db > 0, "pram_retr_plan: needs n_db > 0");
    PRAM_REQUIRE(batch >= 0 && n_frames >= 0 && n_valid >= 0, "pram_retr_plan: needs batch >= 0, n_frames >= 0, n_valid >= 0");
    PRAM_REQUIRE((long long)batch * n_db < 2147483647LL / PRAM_CAND_PLAN_COLS, "pram_retr_plan: batch * n_db does not fit the plan's 32-bit offsets");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(retr_plan_kernel, dim3(cdiv(batch * n_db, 256)), dim3(256), 0, (hipStream_t)stream, retrieval, counts, enable, frame_off,
                       valid_off, batch, n_db, n_frames, n_valid, plan);
    return pram_launch_status("pram_retr_plan");
}

extern "C" int pram_retr_filter(const long long* r_kpt_ids, const float* r_kpts, const float* r_ref_kpts, const long long* r_point3d_ids,
                                const double* r_xyz, const int* r_sids, const int* r_count, int pairs, int t0, const long long* pt_ids,
                                const int* pt_off, int n_points, int obs_th, long long* m_kpt_ids, float* m_kpts, float* m_ref_kpts,
                                long long* m_point3d_ids, double* m_xyz, int* m_sids, int* m_count, void* stream) {
    PRAM_REQUIRE(r_kpt_ids && r_kpts && r_ref_kpts && r_point3d_ids && r_xyz && r_sids && r_count && pt_ids && pt_off && m_kpt_ids && m_kpts &&
                 m_ref_kpts && m_point3d_ids && m_xyz && m_sids && m_count, "pram_retr_filter: null pointer");
    PRAM_REQUIRE(aligned(r_kpt_ids, 8) && aligned(r_point3d_ids, 8) && aligned(r_xyz, 8) && aligned(pt_ids, 8) && aligned(m_kpt_ids, 8) &&
                 aligned(m_point3d_ids, 8) && aligned(m_xyz, 8), "pram_retr_filter: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(r_kpts, 4) && aligned(r_ref_kpts, 4) && aligned(r_sids, 4) && aligned(r_count, 4) && aligned(pt_off, 4) &&
                 aligned(m_kpts, 4) && aligned(m_ref_kpts, 4) && aligned(m_sids, 4) && aligned(m_count, 4), "pram_retr_filter: misaligned pointer");
    PRAM_REQUIRE(pairs >= 0 && t0 >= 0 && n_points >= 0, "pram_retr_filter: needs pairs >= 0, t0 >= 0, n_points >= 0");
    PRAM_REQUIRE(r_kpt_ids != m_kpt_ids && r_point3d_ids != m_point3d_ids, "pram_retr_filter: the filtered list must not be the input");
    if (pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(retr_filter_kernel, dim3(pairs), dim3(256), 0, (hipStream_t)stream,
                       match_list(r_kpt_ids, r_kpts, r_ref_kpts, r_point3d_ids, r_xyz, r_sids), r_count, t0, pt_ids, pt_off, n_points, obs_th,
                       match_list(m_kpt_ids, m_kpts, m_ref_kpts, m_point3d_ids, m_xyz, m_sids), m_count);
    return pram_launch_status("pram_retr_filter");
}

extern "C" int pram_retr_select(const int* success, const int* num_inliers, const int* count, int batch, int n_db, int inlier_th,
                                int min_best_inliers, int* chosen, void* stream) {
    PRAM_REQUIRE(success && num_inliers && count && chosen, "pram_retr_select: null pointer");
    PRAM_REQUIRE(aligned(success, 4) && aligned(num_inliers, 4) && aligned(count, 4) && aligned(chosen, 4), "pram_retr_select: misaligned pointer");
    PRAM_REQUIRE(n_db > 0, "pram_retr_select: needs n_db > 0");
    PRAM_REQUIRE(batch >= 0 && (long long)batch * n_db < 2147483647LL, "pram_retr_select: needs batch >= 0 and batch * n_db below 2^31");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(retr_select_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, (hipStream_t)stream, success, num_inliers, count, batch, n_db,
                       inlier_th, min_best_inliers, chosen);
    return pram_launch_status("pram_retr_select");
}

extern "C" int pram_covis_topk(const int* frames, int n, const int* valid_off, const int* valid_rows, const long long* point3d_ids, int n_rows,
                               int n_valid, const long long* pt_ids, const int* pt_off, const int* pt_frames, int n_points, int n_entries,
                               int n_frames, int k, int include_self, int* hist, int* best_frames, int* best_counts, int* n_found,
                               void* stream) {
    PRAM_REQUIRE(frames && valid_off && valid_rows && point3d_ids && pt_ids && pt_off && pt_frames && hist && best_frames && best_counts &&
                 n_found, "pram_covis_topk: null pointer");
    PRAM_REQUIRE(aligned(point3d_ids, 8) && aligned(pt_ids, 8), "pram_covis_topk: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(frames, 4) && aligned(valid_off, 4) && aligned(valid_rows, 4) && aligned(pt_off, 4) && aligned(pt_frames, 4) &&
                 aligned(hist, 4) && aligned(best_frames, 4) && aligned(best_counts, 4) && aligned(n_found, 4), "pram_covis_topk: misaligned pointer");
    PRAM_REQUIRE(k >= 1, "pram_covis_topk: needs k >= 1");
    PRAM_REQUIRE(n >= 0 && n_rows >= 0 && n_valid >= 0 && n_points >= 0 && n_entries >= 0 && n_frames >= 1,
                 "pram_covis_topk: needs n >= 0, n_rows >= 0, n_valid >= 0, n_points >= 0, n_entries >= 0, n_frames >= 1");
    PRAM_REQUIRE((long long)n * k < 2147483647LL, "pram_covis_topk: n * k overflows");
    if (n == 0) return PRAM_OK;
    if (hipMemsetD32Async((hipDeviceptr_t)hist, 0, (size_t)n * n_frames, (hipStream_t)stream) != hipSuccess)
        return pram_launch_status("pram_covis_topk");
    hipLaunchKernelGGL(covis_topk_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, frames, valid_off, valid_rows, point3d_ids, n_rows, n_valid,
                       pt_ids, pt_off, pt_frames, n_points, n_entries, n_frames, k, include_self != 0, hist, best_frames, best_counts, n_found);
    return pram_launch_status("pram_covis_topk");
}
