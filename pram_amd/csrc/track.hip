// Tracking the last frame (Tracker.track_last_frame localization/tracker.py:162-233, Frame.initialize_localization_variables and
// update_point3ds frame.py:84-89, 191-195, the hand-over mTracker.last_frame = curr_frame loc_by_rec_online.py:193-197) for a
// batch of independent streams: the last frame of every stream stays on the device in a slot of a TrackState (rows slot * n_max
// .. + n_max of every array), a tracking pair is a row of the candidate stage's plan table ("all keypoints of the query" against
// "the rows of the slot"), so pram_cand_gather runs on pram_track_plan's table unchanged with the state's arrays as its
// reference side.  Latency / bandwidth kernels: 16-byte accesses on the descriptor rows, plain vector loads and stores
// elsewhere, one integer atomic max (its result does not depend on the order the rows arrive in), nothing allocated.
#include "glue.h"

namespace {

// one thread per pair
__global__ __launch_bounds__(256) void track_plan_kernel(const int* __restrict__ counts, const int* __restrict__ slot,
                                                         const int* __restrict__ st_counts, const int* __restrict__ st_ref_frame,
                                                         int batch, int n, int n_slots, int n_max, int* __restrict__ plan,
                                                         int* __restrict__ loc_plan) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    const int s = slot[b];
    const bool live = s >= 0 && s < n_slots;
    int nq = counts[b];
    nq = nq < 0 ? 0 : (nq > n ? n : nq);
    int nr = live ? st_counts[s] : 0;
    nr = nr < 0 ? 0 : (nr > n_max ? n_max : nr);
    int* col = plan + b;      // column-major tables: field X of pair b at table[X * batch + b]
    int* lcol = loc_plan + b;
    col[PL_QUERY * batch] = b; col[PL_SID * batch] = -1; col[PL_FRAME * batch] = live ? s : -1; col[PL_SEM * batch] = 0;
    col[PL_LEN0 * batch] = live ? nq : 0; col[PL_LEN1 * batch] = nr; col[PL_TOK_OFF * batch] = -1;
    col[PL_ROW0 * batch] = live ? s * n_max : 0; col[PL_SEL_OFF * batch] = -1; col[PL_ORDER * batch] = 0;
    lcol[PL_QUERY * batch] = b; lcol[PL_SID * batch] = -1; lcol[PL_FRAME * batch] = live ? st_ref_frame[s] : -1; lcol[PL_SEM * batch] = 0;
    lcol[PL_LEN0 * batch] = live ? nq : 0; lcol[PL_LEN1 * batch] = nr; lcol[PL_TOK_OFF * batch] = -1;
    lcol[PL_ROW0 * batch] = live ? s * n_max : 0; lcol[PL_SEL_OFF * batch] = -1; lcol[PL_ORDER * batch] = 0;
}

// one workgroup per pair: the matched query rows whose row of the last frame carries a point (tracker.py:195-205)
__global__ __launch_bounds__(256) void track_correspond_kernel(const long long* __restrict__ matches0, int ldm, const int* __restrict__ plan,
                                                               const float* __restrict__ q_kpts, int n, const float* __restrict__ st_kpts,
                                                               const long long* __restrict__ st_xyz, const long long* __restrict__ st_p3d,
                                                               const int* __restrict__ st_segs, int n_slots, int n_max, int t0, int cap,
                                                               MatchList m, int* __restrict__ m_count) {
    __shared__ int wsum[4];
    const int p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    const int* pl = plan + p;
    const int s = pl[PL_FRAME * P], b = pl[PL_QUERY * P];
    const bool live = s >= 0 && s < n_slots && b >= 0 && b < P;      // uniform over the workgroup
    int len0 = live ? pl[PL_LEN0 * P] : 0;
    len0 = len0 > t0 ? t0 : len0;
    len0 = len0 > n ? n : len0;
    int len1 = pl[PL_LEN1 * P];
    len1 = len1 > n_max ? n_max : len1;
    int base = 0;      // a running sum every thread carries
    for (int c0 = 0; c0 < len0; c0 += 256) {
        const int i = c0 + tid;
        size_t rr = 0;
        bool f = false;
        if (i < len0) {
            const long long j = matches0[(size_t)p * ldm + i];
            if (j >= 0 && j < len1) {
                rr = (size_t)s * n_max + (size_t)j;
                f = st_p3d[rr] >= 0;
            }
        }
        int tot;
        const int o = base + chunk_offset<4>(f, wsum, tot);
        if (f && o < cap) match_emit_row(m, (size_t)p * cap + o, i, q_kpts + ((size_t)b * n + i) * 2, st_kpts, st_p3d, st_xyz, st_segs, rr);
        base += tot;
    }
    if (tid == 0) m_count[p] = base < cap ? base : cap;
}

// one workgroup per query: the rows r < count[b] with mask != 0, in order (tracker.py:154-160)
__global__ __launch_bounds__(256) void track_filter_kernel(ConstMatchList in, const int* __restrict__ count, const unsigned char* __restrict__ mask,
                                                           int cap, MatchList out, int* __restrict__ o_count) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int cnt = count[b];
    cnt = cnt < 0 ? 0 : (cnt > cap ? cap : cnt);
    int base = 0;
    for (int c0 = 0; c0 < cnt; c0 += 256) {
        const int r = c0 + tid;
        const size_t q = (size_t)b * cap + r;
        const bool f = r < cnt && mask[q] != 0;
        int tot;
        const int o = base + chunk_offset<4>(f, wsum, tot);
        if (f) match_copy_row(out, (size_t)b * cap + o, in, q);      // o <= r < cap
        base += tot;
    }
    if (tid == 0) o_count[b] = base;
}

// the new frame into its slot, one wave per row; grid (ceil(n_max / 4), batch).  Rows r < counts[b] take the query's keypoint,
// score and descriptor; ALL n_max rows lose their point (initialize_localization_variables); winner [b][r < n] = -1.
__global__ __launch_bounds__(256) void track_commit_rows_kernel(const float* __restrict__ q_kpts, const float* __restrict__ q_scores,
                                                                const float* __restrict__ q_desc, const int* __restrict__ counts,
                                                                const int* __restrict__ seg_ids, const int* __restrict__ slot,
                                                                const int* __restrict__ ref_frame, int n, float cx, float cy, float sc,
                                                                float* __restrict__ st_kpts, float* __restrict__ st_scores,
                                                                float* __restrict__ st_desc, int* __restrict__ st_counts,
                                                                long long* __restrict__ st_xyz, long long* __restrict__ st_p3d,
                                                                int* __restrict__ st_segs, int* __restrict__ st_ref_frame,
                                                                float* __restrict__ st_frame_norm, int n_slots, int n_max,
                                                                int* __restrict__ winner) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r < n && lane == 40) winner[(size_t)b * n + r] = -1;
    const int s = slot[b];
    if (s < 0 || s >= n_slots || r >= n_max) return;
    int cnt = counts[b];
    cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    const size_t dst = (size_t)s * n_max + r, src = (size_t)b * n + r;
    if (r < cnt) {
        if (lane < 32) reinterpret_cast<f32x4*>(st_desc + dst * 128)[lane] = reinterpret_cast<const f32x4*>(q_desc + src * 128)[lane];
        else if (lane < 34) st_kpts[dst * 2 + (lane - 32)] = q_kpts[src * 2 + (lane - 32)];
        else if (lane == 34) st_scores[dst] = q_scores[src];
    }
    if (lane >= 35 && lane < 38) st_xyz[dst * 3 + (lane - 35)] = 0;      // the bits of +0.0
    else if (lane == 38) st_p3d[dst] = -1;
    else if (lane == 39) st_segs[dst] = (seg_ids != nullptr && r < cnt) ? seg_ids[src] : -1;
    if (r == 0) {
        if (lane == 41) st_counts[s] = cnt;
        else if (lane == 42) st_ref_frame[s] = ref_frame[b];
        else if (lane == 43) st_frame_norm[(size_t)s * 3] = cx;
        else if (lane == 44) st_frame_norm[(size_t)s * 3 + 1] = cy;
        else if (lane == 45) st_frame_norm[(size_t)s * 3 + 2] = sc;
    }
}

// update_point3ds, one workgroup per query: of the list rows naming one keypoint the LAST in list order writes (numpy's fancy
// assignment), whatever order the rows are visited in
__global__ __launch_bounds__(256) void track_commit_scatter_kernel(const int* __restrict__ counts, const int* __restrict__ slot, int n,
                                                                   const long long* __restrict__ m_ids, const long long* __restrict__ m_p3d,
                                                                   const long long* __restrict__ m_xyz, const int* __restrict__ m_sids,
                                                                   const int* __restrict__ m_count, const unsigned char* __restrict__ mask,
                                                                   int cap, long long* __restrict__ st_xyz, long long* __restrict__ st_p3d,
                                                                   int* __restrict__ st_segs, int n_slots, int n_max, int* winner) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s = slot[b];
    if (s < 0 || s >= n_slots) return;      // uniform over the workgroup
    int cnt = counts[b];
    cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    int m = m_count[b];
    m = m < 0 ? 0 : (m > cap ? cap : m);
    int* win = winner + (size_t)b * n;
    for (int r = tid; r < m; r += 256) {
        const size_t row = (size_t)b * cap + r;
        if (mask != nullptr && !mask[row]) continue;
        const long long id = m_ids[row];
        if (id >= 0 && id < cnt) atomicMax(&win[id], r);
    }
    __threadfence();
    __syncthreads();
    for (int r = tid; r < m; r += 256) {
        const size_t row = (size_t)b * cap + r;
        if (mask != nullptr && !mask[row]) continue;
        const long long id = m_ids[row];
        if (id < 0 || id >= cnt) continue;
        // read past this compute unit's vector cache: the maxima were formed by atomics in the L2
        if (__hip_atomic_load(&win[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != r) continue;
        const size_t dst = (size_t)s * n_max + (size_t)id;      // id < cnt <= n <= n_max
        st_xyz[dst * 3] = m_xyz[row * 3]; st_xyz[dst * 3 + 1] = m_xyz[row * 3 + 1]; st_xyz[dst * 3 + 2] = m_xyz[row * 3 + 2];
        st_p3d[dst] = m_p3d[row];
        st_segs[dst] = m_sids[row];
    }
}

}  // namespace

extern "C" int pram_track_plan(const int* counts, const int* slot, const int* st_counts, const int* st_ref_frame, int batch, int n,
                               int n_slots, int n_max, int* plan, int* loc_plan, void* stream) {
    PRAM_REQUIRE(counts && slot && st_counts && st_ref_frame && plan && loc_plan, "pram_track_plan: null pointer");
    PRAM_REQUIRE(aligned(counts, 4) && aligned(slot, 4) && aligned(st_counts, 4) && aligned(st_ref_frame, 4) && aligned(plan, 4) &&
                 aligned(loc_plan, 4), "pram_track_plan: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && n >= 0 && n_slots >= 0 && n_max >= 0, "pram_track_plan: needs batch >= 0, n >= 0, n_slots >= 0, n_max >= 0");
    PRAM_REQUIRE((long long)n_slots * n_max < 2147483647LL && (long long)batch < 2147483647LL / PRAM_CAND_PLAN_COLS,
                 "pram_track_plan: n_slots * n_max or batch does not fit the plan's 32-bit offsets");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(track_plan_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, (hipStream_t)stream, counts, slot, st_counts, st_ref_frame, batch,
                       n, n_slots, n_max, plan, loc_plan);
    return pram_launch_status("pram_track_plan");
}

extern "C" int pram_track_correspond(const long long* matches0, int ldm, const int* plan, const float* q_kpts, int n, const float* st_kpts,
                                     const double* st_xyz, const long long* st_point3d_ids, const int* st_segs, int n_slots, int n_max,
                                     int pairs, int t0, int cap, long long* m_kpt_ids, float* m_kpts, float* m_ref_kpts,
                                     long long* m_point3d_ids, double* m_xyz, int* m_sids, int* m_count, void* stream) {
    PRAM_REQUIRE(matches0 && plan && q_kpts && st_kpts && st_xyz && st_point3d_ids && st_segs && m_kpt_ids && m_kpts && m_ref_kpts &&
                 m_point3d_ids && m_xyz && m_sids && m_count, "pram_track_correspond: null pointer");
    PRAM_REQUIRE(aligned(matches0, 8) && aligned(st_xyz, 8) && aligned(st_point3d_ids, 8) && aligned(m_kpt_ids, 8) && aligned(m_point3d_ids, 8) &&
                 aligned(m_xyz, 8), "pram_track_correspond: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(plan, 4) && aligned(q_kpts, 4) && aligned(st_kpts, 4) && aligned(st_segs, 4) && aligned(m_kpts, 4) && aligned(m_ref_kpts, 4) &&
                 aligned(m_sids, 4) && aligned(m_count, 4), "pram_track_correspond: misaligned pointer");
    PRAM_REQUIRE(pairs >= 0 && t0 >= 0 && ldm >= t0 && cap >= 0 && n >= 0 && n_slots >= 0 && n_max >= 0,
                 "pram_track_correspond: needs pairs >= 0, 0 <= t0 <= ldm, cap >= 0, n >= 0, n_slots >= 0, n_max >= 0");
    if (pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(track_correspond_kernel, dim3(pairs), dim3(256), 0, (hipStream_t)stream, matches0, ldm, plan, q_kpts, n, st_kpts,
                       reinterpret_cast<const long long*>(st_xyz), st_point3d_ids, st_segs, n_slots, n_max, t0, cap,
                       match_list(m_kpt_ids, m_kpts, m_ref_kpts, m_point3d_ids, m_xyz, m_sids), m_count);
    return pram_launch_status("pram_track_correspond");
}

extern "C" int pram_track_filter(const long long* kpt_ids, const float* kpts, const float* ref_kpts, const long long* point3d_ids,
                                 const double* xyz, const int* sids, const int* count, const unsigned char* mask, int batch, int cap,
                                 long long* o_kpt_ids, float* o_kpts, float* o_ref_kpts, long long* o_point3d_ids, double* o_xyz,
                                 int* o_sids, int* o_count, void* stream) {
    PRAM_REQUIRE(kpt_ids && kpts && ref_kpts && point3d_ids && xyz && sids && count && mask && o_kpt_ids && o_kpts && o_ref_kpts &&
                 o_point3d_ids && o_xyz && o_sids && o_count, "pram_track_filter: null pointer");
    PRAM_REQUIRE(aligned(kpt_ids, 8) && aligned(point3d_ids, 8) && aligned(xyz, 8) && aligned(o_kpt_ids, 8) && aligned(o_point3d_ids, 8) &&
                 aligned(o_xyz, 8), "pram_track_filter: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(kpts, 4) && aligned(ref_kpts, 4) && aligned(sids, 4) && aligned(count, 4) && aligned(o_kpts, 4) && aligned(o_ref_kpts, 4) &&
                 aligned(o_sids, 4) && aligned(o_count, 4), "pram_track_filter: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && cap >= 0, "pram_track_filter: needs batch >= 0, cap >= 0");
    PRAM_REQUIRE((const void*)kpt_ids != (const void*)o_kpt_ids && (const void*)kpts != (const void*)o_kpts && (const void*)ref_kpts != (const void*)o_ref_kpts &&
                 (const void*)point3d_ids != (const void*)o_point3d_ids && (const void*)xyz != (const void*)o_xyz && (const void*)sids != (const void*)o_sids,
                 "pram_track_filter: the output lists must not be the input lists");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(track_filter_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, match_list(kpt_ids, kpts, ref_kpts, point3d_ids, xyz, sids),
                       count, mask, cap, match_list(o_kpt_ids, o_kpts, o_ref_kpts, o_point3d_ids, o_xyz, o_sids), o_count);
    return pram_launch_status("pram_track_filter");
}

extern "C" int pram_track_commit(const float* q_kpts, const float* q_scores, const float* q_desc, const int* counts, const int* seg_ids,
                                 const int* slot, const int* slot_host, const int* ref_frame, int batch, int n, float q_cx, float q_cy,
                                 float q_scale, const long long* m_kpt_ids, const long long* m_point3d_ids, const double* m_xyz,
                                 const int* m_sids, const int* m_count, const unsigned char* mask, int cap, float* st_kpts,
                                 float* st_scores, float* st_desc, int* st_counts, double* st_xyz, long long* st_point3d_ids, int* st_segs,
                                 int* st_ref_frame, float* st_frame_norm, int n_slots, int n_max, int* winner, void* stream) {
    PRAM_REQUIRE(q_kpts && q_scores && q_desc && counts && slot && slot_host && ref_frame && m_kpt_ids && m_point3d_ids && m_xyz && m_sids &&
                 m_count && st_kpts && st_scores && st_desc && st_counts && st_xyz && st_point3d_ids && st_segs && st_ref_frame && st_frame_norm &&
                 winner, "pram_track_commit: null pointer");
    PRAM_REQUIRE(aligned(q_desc, 16) && aligned(st_desc, 16), "pram_track_commit: descriptor buffers must be 16-byte aligned");
    PRAM_REQUIRE(aligned(m_kpt_ids, 8) && aligned(m_point3d_ids, 8) && aligned(m_xyz, 8) && aligned(st_xyz, 8) && aligned(st_point3d_ids, 8),
                 "pram_track_commit: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(q_kpts, 4) && aligned(q_scores, 4) && aligned(counts, 4) && aligned(seg_ids, 4) && aligned(slot, 4) && aligned(slot_host, 4) &&
                 aligned(ref_frame, 4) && aligned(m_sids, 4) && aligned(m_count, 4) && aligned(st_kpts, 4) && aligned(st_scores, 4) &&
                 aligned(st_counts, 4) && aligned(st_segs, 4) && aligned(st_ref_frame, 4) && aligned(st_frame_norm, 4) && aligned(winner, 4),
                 "pram_track_commit: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && batch <= 65535 && n >= 0 && cap >= 0 && n_slots >= 0 && n_max >= 0 && n <= n_max && q_scale > 0.f,
                 "pram_track_commit: needs 0 <= batch <= 65535, 0 <= n <= n_max, cap >= 0, n_slots >= 0, q_scale > 0");
    PRAM_REQUIRE((long long)n_slots * n_max < 2147483647LL, "pram_track_commit: n_slots * n_max overflows");
    for (int b = 0; b < batch; ++b) {      // a host copy, checked here without touching the device
        const int s = slot_host[b];
        if (s < 0) continue;
        PRAM_REQUIRE(s < n_slots, "pram_track_commit: slot %d of query %d is outside the state's %d slots", s, b, n_slots);
        for (int a = 0; a < b; ++a)
            PRAM_REQUIRE(slot_host[a] != s, "pram_track_commit: queries %d and %d name one slot (%d)", a, b, s);
    }
    if (batch == 0) return PRAM_OK;
    const int rows = n_max > n ? n_max : n;
    if (rows > 0)
        hipLaunchKernelGGL(track_commit_rows_kernel, dim3(cdiv(rows, 4), batch), dim3(256), 0, (hipStream_t)stream, q_kpts, q_scores, q_desc, counts,
                           seg_ids, slot, ref_frame, n, q_cx, q_cy, q_scale, st_kpts, st_scores, st_desc, st_counts,
                           reinterpret_cast<long long*>(st_xyz), st_point3d_ids, st_segs, st_ref_frame, st_frame_norm, n_slots, n_max, winner);
    if (n > 0 && cap > 0)
        hipLaunchKernelGGL(track_commit_scatter_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, counts, slot, n, m_kpt_ids, m_point3d_ids,
                           reinterpret_cast<const long long*>(m_xyz), m_sids, m_count, mask, cap, reinterpret_cast<long long*>(st_xyz),
                           st_point3d_ids, st_segs, n_slots, n_max, winner);
    return pram_launch_status("pram_track_commit");
}
