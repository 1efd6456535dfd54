// Pose refinement by matching over covisible frames (SingleMap3D.refine_pose_by_matching singlemap3d.py:268-365, its frame vote
// find_reference_frames singlemap3d.py:500-511): the glue around the grouped matcher call.  A refinement pair is a plan row of
// the candidate stage ("all keypoints of the query" against "the whole frame"), so pram_cand_gather / pram_cand_correspond run on
// the plan written here unchanged.  Latency / bandwidth kernels: plain vector loads and stores, integer atomics only (the results
// do not depend on the order the adds arrive in), every loop bounded by an argument, nothing allocated.
#include "glue.h"

namespace {

// one thread per (query b, slot j < n_cov); the thread of slot 0 also writes the query's own row
__global__ __launch_bounds__(256) void refine_plan_kernel(const int* __restrict__ chosen, const int* __restrict__ loc_plan,
                                                          const int* __restrict__ counts, const int* __restrict__ enable,
                                                          const int* __restrict__ frame_off, const int* __restrict__ covis_off,
                                                          const int* __restrict__ covis_frames, int batch, int seg_k, int n_cov,
                                                          int n_frames, int n_covis, int* __restrict__ plan, int* __restrict__ ref_frame,
                                                          int* __restrict__ n_cov_used, int* __restrict__ init_on) {
    const int p = blockIdx.x * 256 + threadIdx.x, pairs = batch * n_cov;
    if (p >= pairs) return;
    const int b = p / n_cov, j = p - b * n_cov;
    const int kept = chosen[b * 3], status = chosen[b * 3 + 1];
    const int sid = (kept >= 0 && kept < seg_k) ? loc_plan[PL_SID * batch * seg_k + b * seg_k + kept] : -1;
    // the covisible list of the localisation's reference frame, cut to n_cov (the canonical order makes it a prefix)
    const Slots s = query_slots(chosen, loc_plan, enable, covis_off, b, batch, seg_k, n_cov, n_frames, n_covis);
    const int f = s.f, c0 = s.c0, len = s.len;      // not live: f = -1 and an empty list
    int g = j < len ? covis_frames[c0 + j] : -1;
    if (g >= n_frames) g = -1;
    int nq = counts[b];
    nq = nq < 0 ? 0 : nq;
    int* col = plan + p;      // column-major table: field X of pair p at plan[X * pairs + p]
    const int row0 = g >= 0 ? frame_off[g] : 0;
    col[PL_QUERY * pairs] = b; col[PL_SID * pairs] = sid; col[PL_FRAME * pairs] = g; col[PL_SEM * pairs] = 0;
    col[PL_LEN0 * pairs] = g >= 0 ? nq : 0;
    col[PL_LEN1 * pairs] = g >= 0 ? frame_off[g + 1] - row0 : 0;
    col[PL_TOK_OFF * pairs] = -1; col[PL_ROW0 * pairs] = row0; col[PL_SEL_OFF * pairs] = -1; col[PL_ORDER * pairs] = j;
    if (j == 0) {
        int in_list = 0;
        for (int i = 0; i < len; ++i) in_list |= covis_frames[c0 + i] == f;      // singlemap3d.py:273 "ref_frame_id in db_ids"
        ref_frame[b] = f;
        n_cov_used[b] = len;
        init_on[b] = f >= 0 && status == 1 && in_list;
    }
}

// one workgroup per query: the slots in ascending order, then the localisation's matches (singlemap3d.py:288-315)
__global__ __launch_bounds__(256) void refine_merge_kernel(ConstMatchList r, const int* __restrict__ r_count, int t0, ConstMatchList a,
                                                           const int* __restrict__ a_count, int t0a, const int* __restrict__ chosen,
                                                           const int* __restrict__ init_on, int seg_k, int n_cov, int cap, MatchList m,
                                                           int* __restrict__ m_src, int* __restrict__ m_count) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int kept = chosen[b * 3];
    const bool with_init = init_on[b] != 0 && kept >= 0 && kept < seg_k;
    // exclusive scan of the segment counts: a running sum every thread carries (the counts are uniform over the workgroup), so an
    // empty slot costs one load
    int base = 0;
    for (int s = 0; s <= n_cov; ++s) {
        const bool init = s == n_cov;
        if (init && !with_init) break;
        const ConstMatchList& src = init ? a : r;
        const int ld = init ? t0a : t0;
        const size_t seg = init ? (size_t)(b * seg_k + kept) : (size_t)b * n_cov + s;
        int cnt = init ? a_count[seg] : r_count[seg];
        cnt = cnt < 0 ? 0 : (cnt > ld ? ld : cnt);
        if (base + cnt > cap) cnt = cap - base;
        for (int i = tid; i < cnt; i += 256) {
            const size_t q = seg * ld + i, d = (size_t)b * cap + base + i;
            match_copy_row(m, d, src, q);
            m_src[d] = s;
        }
        base += cnt;
    }
    if (tid == 0) m_count[b] = base;
}

// one workgroup per query: the vote into hist [batch][n_frames] (global memory, zeroed by the entry), then k selection rounds
__global__ __launch_bounds__(256) void refine_frame_vote_kernel(const long long* __restrict__ m_p3d, const int* __restrict__ m_count,
                                                                const unsigned char* __restrict__ inliers, const int* __restrict__ success,
                                                                int cap, const long long* __restrict__ pt_ids, const int* __restrict__ pt_off,
                                                                const int* __restrict__ pt_frames, int n_points, int n_entries,
                                                                const int* __restrict__ is_vrf, int n_frames, int k, int* hist,
                                                                int* __restrict__ best_frames, int* __restrict__ best_counts,
                                                                int* __restrict__ n_best) {
    __shared__ unsigned long long wbest[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = m_count[b];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const bool only_inliers = success[b] != 0;
    int* h = hist + (size_t)b * n_frames;
    for (int r = tid; r < n; r += 256) {
        const size_t row = (size_t)b * cap + r;
        if (only_inliers && !inliers[row]) continue;
        const long long id = m_p3d[row];
        const int lo = lower_bound_i64(pt_ids, n_points, id);
        if (lo >= n_points || pt_ids[lo] != id) continue;      // a point the map does not know votes for nothing
        int e0 = pt_off[lo], e1 = pt_off[lo + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > n_entries ? n_entries : e1;
        for (int e = e0; e < e1; ++e) {
            const int f = pt_frames[e];
            if (f >= 0 && f < n_frames && is_vrf[f]) atomicAdd(&h[f], 1);
        }
    }
    __threadfence();
    __syncthreads();
    // round r takes the largest (count, then smaller frame index) strictly after round r - 1's pick; the counts are read past this
    // compute unit's vector cache, which may hold a line of a neighbouring query's histogram from before the adds
    unsigned long long prev = ~0ull;
    int found = 0;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = 0;
        for (int f = tid; f < n_frames; f += 256) {
            const int c = __hip_atomic_load(&h[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)(0x7fffffff - f);
            if (c > 0 && key < prev && key > best) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other > best ? other : best;
        }
        if (lane == 0) wbest[wave] = best;
        __syncthreads();
        best = wbest[0];
        for (int w = 1; w < 4; ++w) best = wbest[w] > best ? wbest[w] : best;
        __syncthreads();
        if (best != 0) { prev = best; ++found; }
        else prev = 0;      // nothing left: every later round finds nothing either
        if (tid == 0) {
            best_frames[(size_t)b * k + r] = best ? 0x7fffffff - (int)(best & 0xffffffffu) : -1;
            best_counts[(size_t)b * k + r] = (int)(best >> 32);
        }
    }
    if (tid == 0) n_best[b] = found;
}

}  // namespace

extern "C" int pram_refine_plan(const int* chosen, const int* loc_plan, const int* counts, const int* enable, const int* frame_off,
                                const int* covis_off, const int* covis_frames, int batch, int seg_k, int n_cov, int n_frames,
                                int n_covis, int* plan, int* ref_frame, int* n_cov_used, int* init_on, void* stream) {
    PRAM_REQUIRE(chosen && loc_plan && counts && frame_off && covis_off && covis_frames && plan && ref_frame && n_cov_used && init_on,
                 "pram_refine_plan: null pointer");
    PRAM_REQUIRE(aligned(chosen, 4) && aligned(loc_plan, 4) && aligned(counts, 4) && aligned(enable, 4) && aligned(frame_off, 4) &&
                 aligned(covis_off, 4) && aligned(covis_frames, 4) && aligned(plan, 4) && aligned(ref_frame, 4) && aligned(n_cov_used, 4) &&
                 aligned(init_on, 4), "pram_refine_plan: misaligned pointer");
    PRAM_REQUIRE(n_cov > 0, "pram_refine_plan: needs n_cov > 0");
    PRAM_REQUIRE(batch >= 0 && seg_k >= 1 && n_frames >= 0 && n_covis >= 0, "pram_refine_plan: needs batch >= 0, seg_k >= 1, n_frames >= 0, n_covis >= 0");
    PRAM_REQUIRE((long long)batch * n_cov < 2147483647LL / PRAM_CAND_PLAN_COLS && (long long)batch * seg_k < 2147483647LL / PRAM_CAND_PLAN_COLS,
                 "pram_refine_plan: batch * n_cov or batch * seg_k does not fit the plan's 32-bit offsets");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(refine_plan_kernel, dim3(cdiv(batch * n_cov, 256)), dim3(256), 0, (hipStream_t)stream, chosen, loc_plan, counts, enable,
                       frame_off, covis_off, covis_frames, batch, seg_k, n_cov, n_frames, n_covis, plan, ref_frame, n_cov_used, init_on);
    return pram_launch_status("pram_refine_plan");
}

extern "C" int pram_refine_merge(const long long* r_kpt_ids, const float* r_kpts, const float* r_ref_kpts, const long long* r_point3d_ids,
                                 const double* r_xyz, const int* r_sids, const int* r_count, int t0, const long long* a_kpt_ids,
                                 const float* a_kpts, const float* a_ref_kpts, const long long* a_point3d_ids, const double* a_xyz,
                                 const int* a_sids, const int* a_count, int t0a, const int* chosen, const int* init_on, int batch,
                                 int seg_k, int n_cov, int cap, long long* m_kpt_ids, float* m_kpts, float* m_ref_kpts,
                                 long long* m_point3d_ids, double* m_xyz, int* m_sids, int* m_src, int* m_count, void* stream) {
    PRAM_REQUIRE(r_kpt_ids && r_kpts && r_ref_kpts && r_point3d_ids && r_xyz && r_sids && r_count && a_kpt_ids && a_kpts && a_ref_kpts &&
                 a_point3d_ids && a_xyz && a_sids && a_count && chosen && init_on && m_kpt_ids && m_kpts && m_ref_kpts && m_point3d_ids &&
                 m_xyz && m_sids && m_src && m_count, "pram_refine_merge: null pointer");
    PRAM_REQUIRE(aligned(r_kpt_ids, 8) && aligned(r_point3d_ids, 8) && aligned(r_xyz, 8) && aligned(a_kpt_ids, 8) && aligned(a_point3d_ids, 8) &&
                 aligned(a_xyz, 8) && aligned(m_kpt_ids, 8) && aligned(m_point3d_ids, 8) && aligned(m_xyz, 8),
                 "pram_refine_merge: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(r_kpts, 4) && aligned(r_ref_kpts, 4) && aligned(r_sids, 4) && aligned(r_count, 4) && aligned(a_kpts, 4) &&
                 aligned(a_ref_kpts, 4) && aligned(a_sids, 4) && aligned(a_count, 4) && aligned(chosen, 4) && aligned(init_on, 4) &&
                 aligned(m_kpts, 4) && aligned(m_ref_kpts, 4) && aligned(m_sids, 4) && aligned(m_src, 4) && aligned(m_count, 4),
                 "pram_refine_merge: misaligned pointer");
    PRAM_REQUIRE(n_cov > 0, "pram_refine_merge: needs n_cov > 0");
    PRAM_REQUIRE(batch >= 0 && seg_k >= 1 && t0 >= 0 && t0a >= 0, "pram_refine_merge: needs batch >= 0, seg_k >= 1, t0 >= 0, t0a >= 0");
    PRAM_REQUIRE((long long)n_cov * t0 + t0a <= (long long)cap && cap < 2147483647, "pram_refine_merge: cap is smaller than n_cov * t0 + t0a");
    PRAM_REQUIRE((long long)batch * n_cov < 2147483647LL && (long long)batch * seg_k < 2147483647LL, "pram_refine_merge: batch * n_cov or batch * seg_k overflows");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(refine_merge_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream,
                       match_list(r_kpt_ids, r_kpts, r_ref_kpts, r_point3d_ids, r_xyz, r_sids), r_count, t0,
                       match_list(a_kpt_ids, a_kpts, a_ref_kpts, a_point3d_ids, a_xyz, a_sids), a_count, t0a, chosen, init_on, seg_k, n_cov, cap,
                       match_list(m_kpt_ids, m_kpts, m_ref_kpts, m_point3d_ids, m_xyz, m_sids), m_src, m_count);
    return pram_launch_status("pram_refine_merge");
}

extern "C" int pram_refine_frame_vote(const long long* m_point3d_ids, const int* m_count, const unsigned char* inliers, const int* success,
                                      int batch, int cap, const long long* pt_ids, const int* pt_off, const int* pt_frames, int n_points,
                                      int n_entries, const int* is_vrf, int n_frames, int k, int* hist, int* best_frames, int* best_counts,
                                      int* n_best, void* stream) {
    PRAM_REQUIRE(m_point3d_ids && m_count && inliers && success && pt_ids && pt_off && pt_frames && is_vrf && hist && best_frames &&
                 best_counts && n_best, "pram_refine_frame_vote: null pointer");
    PRAM_REQUIRE(aligned(m_point3d_ids, 8) && aligned(pt_ids, 8), "pram_refine_frame_vote: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(m_count, 4) && aligned(success, 4) && aligned(pt_off, 4) && aligned(pt_frames, 4) && aligned(is_vrf, 4) &&
                 aligned(hist, 4) && aligned(best_frames, 4) && aligned(best_counts, 4) && aligned(n_best, 4),
                 "pram_refine_frame_vote: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && cap >= 0 && n_points >= 0 && n_entries >= 0 && n_frames >= 0,
                 "pram_refine_frame_vote: needs batch >= 0, cap >= 0, n_points >= 0, n_entries >= 0, n_frames >= 0");
    PRAM_REQUIRE(k >= 1 && k <= n_frames, "pram_refine_frame_vote: needs 1 <= k <= n_frames");
    if (batch == 0) return PRAM_OK;
    if (hipMemsetD32Async((hipDeviceptr_t)hist, 0, (size_t)batch * n_frames, (hipStream_t)stream) != hipSuccess)
        return pram_launch_status("pram_refine_frame_vote");
    hipLaunchKernelGGL(refine_frame_vote_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, m_point3d_ids, m_count, inliers, success, cap,
                       pt_ids, pt_off, pt_frames, n_points, n_entries, is_vrf, n_frames, k, hist, best_frames, best_counts, n_best);
    return pram_launch_status("pram_refine_frame_vote");
}
