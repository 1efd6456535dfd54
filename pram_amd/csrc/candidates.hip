// Candidate-landmark matching glue (MultiMap3D.run localization/multimap3d.py:110-145, SingleMap3D.localize_with_ref_frame
// singlemap3d.py:127-162, check_semantic_consistency singlemap3d.py:513-532, RefFrame.get_keypoints[_by_sid] refframe.py:34-75):
// from the landmark vote of a batch of queries to the grouped matcher's inputs, and from its matches0 to 2D-3D correspondences,
// without a host loop.  Bandwidth / latency kernels: coalesced 16-byte accesses on the descriptor rows, nothing tuned beyond that.
#include "glue.h"

namespace {

constexpr int CAND_MAX_C = 1024;          // classes of the recogniser (pram_seg_vote's own limit)

// sorted class ids of the padded tokens (t >= counts[b]) -> 0 at every rank: background is never a candidate of the vote and a
// token that names it at every rank names no landmark, so pram_seg_vote over all n rows equals the vote over the first counts[b].
__global__ __launch_bounds__(256) void cand_mask_ranks_kernel(long long* __restrict__ idx, const int* __restrict__ counts, int n, int c) {
    const int b = blockIdx.y;
    int cnt = counts[b];
    cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    const size_t total = (size_t)(n - cnt) * c;
    long long* p = idx + ((size_t)b * n + cnt) * c;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) p[i] = 0;
}

// one workgroup per (candidate w, query b).  MAPS = false: the tables of ONE map, indexed by the in-map id (global id - start_sid).
// MAPS = true (a multi-map store): the landmark tables are indexed by the GLOBAL id and lm_start[gsid] is the start_sid of the map
// that owns it (multimap3d.py:119-123: sid_scene_name picks the map, scene_name_start_sid the in-map id); a reference frame at or
// beyond n_frames is an empty pair as well.
template <bool MAPS>
__global__ __launch_bounds__(256) void cand_plan_kernel(const int* __restrict__ win_sid, const int* __restrict__ win_cnt,
                                                        const int* __restrict__ n_win, const int* __restrict__ seg_ids,
                                                        const int* __restrict__ counts, int n, int seg_k,
                                                        const int* __restrict__ lm_frame, const int* __restrict__ lm_sel_off,
                                                        const int* __restrict__ lm_sel_len, int n_landmarks, int start_sid,
                                                        const int* __restrict__ lm_start, int n_frames,
                                                        const int* __restrict__ frame_off, const int* __restrict__ hist_off,
                                                        const int* __restrict__ hist_label, const int* __restrict__ hist_cnt,
                                                        int min_kpts, double overlap_ratio, int semantic_on, int* __restrict__ plan) {
    __shared__ int qhist[CAND_MAX_C + 1];      // query labels -1 .. CAND_MAX_C - 1 at index label + 1
    __shared__ int red[2][4];
    const int w = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pairs = gridDim.y * seg_k;
    int* col = plan + (b * seg_k + w);      // column-major table: field X of pair p at plan[X * pairs + p]
    int nq = counts[b];
    nq = nq < 0 ? 0 : (nq > n ? n : nq);
    int nw = n_win[b];
    nw = nw > seg_k ? seg_k : nw;
    const bool live = w < nw;
    const int gsid = live ? win_sid[b * seg_k + w] - 1 : -1;      // multimap3d.py:119 "start from 0"
    int lsid, lm, f;      // in-map id (multimap3d.py:123), the landmark's index in the tables, its reference frame
    if constexpr (MAPS) {
        lm = gsid;
        f = (live && gsid >= 0 && gsid < n_landmarks) ? lm_frame[gsid] : -1;
        if (f >= n_frames) f = -1;
        start_sid = f >= 0 ? lm_start[gsid] : 0;
        lsid = gsid - start_sid;
    } else {
        lsid = lm = gsid - start_sid;
        f = (live && lsid >= 0 && lsid < n_landmarks) ? lm_frame[lsid] : -1;
    }
    if (f < 0) {      // no such candidate (or a landmark the map has no reference frame for): an empty pair
        if (tid == 0) {
            col[PL_QUERY * pairs] = b; col[PL_SID * pairs] = gsid; col[PL_FRAME * pairs] = -1; col[PL_SEM * pairs] = 0; col[PL_LEN0 * pairs] = 0; col[PL_LEN1 * pairs] = 0;
            col[PL_TOK_OFF * pairs] = -1; col[PL_ROW0 * pairs] = 0; col[PL_SEL_OFF * pairs] = -1; col[PL_ORDER * pairs] = w;
        }
        return;
    }
    int ntok = win_cnt[b * seg_k + w];
    ntok = ntok < 0 ? 0 : (ntok > nq ? nq : ntok);
    const int row0 = frame_off[f], nref = frame_off[f + 1] - row0;
    int sem = 0;
    if (semantic_on && ntok >= min_kpts) {      // uniform over the workgroup
        // check_semantic_consistency: labels both sides carry, the share of each side's keypoints that carry one of them
        for (int i = tid; i <= CAND_MAX_C; i += 256) qhist[i] = 0;
        __syncthreads();
        const int* q = seg_ids + (size_t)b * n;
        for (int t = tid; t < nq; t += 256) {
            const int l = q[t];
            if (l >= -1 && l < CAND_MAX_C) atomicAdd(&qhist[l + 1], 1);
        }
        __syncthreads();
        int num1 = 0, num2 = 0;
        for (int e = hist_off[f] + tid; e < hist_off[f + 1]; e += 256) {
            const long long g = (long long)hist_label[e] + start_sid;
            if (g >= -1 && g < CAND_MAX_C && qhist[g + 1] > 0) { num1 += qhist[g + 1]; num2 += hist_cnt[e]; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { num1 += __shfl_xor(num1, o, 64); num2 += __shfl_xor(num2, o, 64); }
        if (lane == 0) { red[0][wave] = num1; red[1][wave] = num2; }
        __syncthreads();
        num1 = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        num2 = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        const double r1 = (double)num1 / (double)nq, r2 = (double)num2 / (double)nref;
        const double m = (r2 < r1) ? r2 : r1;      // Python's min(ratio1, ratio2)
        sem = m >= overlap_ratio;
    }
    if (tid == 0) {
        const bool by_sid = sem && lsid > 0;        // singlemap3d.py:130
        col[PL_QUERY * pairs] = b; col[PL_SID * pairs] = gsid; col[PL_FRAME * pairs] = f; col[PL_SEM * pairs] = sem;
        col[PL_LEN0 * pairs] = sem ? ntok : nq;
        col[PL_LEN1 * pairs] = by_sid ? lm_sel_len[lm] : nref;
        col[PL_TOK_OFF * pairs] = sem ? (b * seg_k + w) * n : -1;
        col[PL_ROW0 * pairs] = row0;
        col[PL_SEL_OFF * pairs] = by_sid ? lm_sel_off[lm] : -1;
        col[PL_ORDER * pairs] = w;
    }
}

// one wave per output row; grid (ceil(T / 4), 2 P): set s < P = query side of pair s, else reference side of pair s - P
__global__ __launch_bounds__(256) void cand_gather_kernel(const int* __restrict__ plan, const int* __restrict__ tokens,
                                                          const int* __restrict__ sel_rows, const float* __restrict__ q_desc,
                                                          const float* __restrict__ q_kpts, const float* __restrict__ q_scores, int n,
                                                          const float* __restrict__ r_desc, const float* __restrict__ r_kpts,
                                                          const float* __restrict__ r_scores, const float* __restrict__ frame_norm,
                                                          int ref_rows, float qcx, float qcy, float qscale, float* __restrict__ d0,
                                                          float* __restrict__ k0, float* __restrict__ s0, float* __restrict__ d1,
                                                          float* __restrict__ k1, float* __restrict__ s1, int P, int T) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= T) return;
    const int s = blockIdx.y, side = s >= P, p = side ? s - P : s;
    const int* pl = plan + p;
    const float* sd = nullptr; const float* sk = nullptr; const float* ss = nullptr;
    float cx = qcx, cy = qcy, sc = qscale;
    if (!side) {
        if (r < pl[PL_LEN0 * P]) {
            const int off = pl[PL_TOK_OFF * P];
            const int t = off < 0 ? r : tokens[(size_t)off + r];
            if (t >= 0 && t < n) {
                const size_t src = (size_t)pl[PL_QUERY * P] * n + t;
                sd = q_desc + src * 128; sk = q_kpts + src * 2; ss = q_scores + src;
            }
        }
    } else if (r < pl[PL_LEN1 * P]) {
        const int off = pl[PL_SEL_OFF * P];
        const int t = off < 0 ? pl[PL_ROW0 * P] + r : sel_rows[(size_t)off + r];
        if (t >= 0 && t < ref_rows) {
            sd = r_desc + (size_t)t * 128; sk = r_kpts + (size_t)t * 2; ss = r_scores + t;
            const float* fn = frame_norm + (size_t)pl[PL_FRAME * P] * 3;
            cx = fn[0]; cy = fn[1]; sc = fn[2];
        }
    }
    const size_t dst = (size_t)p * T + r;
    float* od = (side ? d1 : d0) + dst * 128;
    float* ok = (side ? k1 : k0) + dst * 2;
    float* os = (side ? s1 : s0) + dst;
    if (lane < 32) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (sd) v = reinterpret_cast<const f32x4*>(sd)[lane];
        reinterpret_cast<f32x4*>(od)[lane] = v;
    } else if (lane < 34) {      // normalize_keypoints, nets/utils.py:17-24: (k - centre) / scale, as pram_fourier_encoding_f32 does it
        const int a = lane - 32;
        ok[a] = sd ? (sk[a] - (a ? cy : cx)) / sc : 0.f;
    } else if (lane == 34) {
        *os = sd ? *ss : 0.f;
    }
}

// one workgroup per pair: ordered compaction of the matched query rows (singlemap3d.py:156-162)
__global__ __launch_bounds__(256) void cand_correspond_kernel(const long long* __restrict__ matches0, int ldm, const int* __restrict__ plan,
                                                              const int* __restrict__ tokens, const int* __restrict__ sel_rows,
                                                              const float* __restrict__ q_kpts, int n, const float* __restrict__ r_kpts,
                                                              const long long* __restrict__ r_xyz, const long long* __restrict__ r_p3d,
                                                              const int* __restrict__ r_segs, int ref_rows, int t0, int cap,
                                                              MatchList m, int* __restrict__ m_count) {
    __shared__ int wsum[4];
    const int p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    const int* pl = plan + p;
    int len0 = pl[PL_LEN0 * P];
    len0 = len0 > t0 ? t0 : len0;
    const int len1 = pl[PL_LEN1 * P], tok_off = pl[PL_TOK_OFF * P], sel_off = pl[PL_SEL_OFF * P], row0 = pl[PL_ROW0 * P], b = pl[PL_QUERY * P];
    int base = 0;      // a running sum every thread carries
    for (int c0 = 0; c0 < len0; c0 += 256) {
        const int i = c0 + tid;
        long long j = -1;
        int qt = -1, rr = -1;
        if (i < len0) {
            j = matches0[(size_t)p * ldm + i];
            if (j >= 0 && j < len1) {
                qt = tok_off < 0 ? i : tokens[(size_t)tok_off + i];
                rr = sel_off < 0 ? row0 + (int)j : sel_rows[(size_t)sel_off + j];
            }
        }
        const bool f = qt >= 0 && qt < n && rr >= 0 && rr < ref_rows;
        int tot;
        const int o = base + chunk_offset<4>(f, wsum, tot);
        if (f && o < cap)
            match_emit_row(m, (size_t)p * cap + o, qt, q_kpts + ((size_t)b * n + qt) * 2, r_kpts, r_p3d, r_xyz, r_segs, (size_t)rr);
        base += tot;
    }
    if (tid == 0) m_count[p] = base < cap ? base : cap;
}

}  // namespace

extern "C" int pram_cand_mask_ranks(long long* sorted_ids, const int* counts, int batch, int n, int c, void* stream) {
    PRAM_REQUIRE(sorted_ids && counts, "pram_cand_mask_ranks: null pointer");
    PRAM_REQUIRE(aligned(sorted_ids, 8) && aligned(counts, 4), "pram_cand_mask_ranks: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && batch <= 65535 && n >= 0 && c > 0 && c <= CAND_MAX_C, "pram_cand_mask_ranks: needs 0 <= batch <= 65535, n >= 0, 0 < classes <= %d", CAND_MAX_C);
    if (batch == 0 || n == 0) return PRAM_OK;
    hipLaunchKernelGGL(cand_mask_ranks_kernel, dim3(16, batch), dim3(256), 0, (hipStream_t)stream, sorted_ids, counts, n, c);
    return pram_launch_status("pram_cand_mask_ranks");
}

namespace {

// the two plan entries: one set of checks and statuses (maps: lm_start is read and start_sid is not; else the other way round)
int cand_plan_launch(const char* what, const int* win_sid, const int* win_count, const int* n_win, const int* seg_ids, const int* counts, int batch,
                     int n, int n_class, int seg_k, const int* lm_frame, const int* lm_sel_off, const int* lm_sel_len, int n_landmarks,
                     int start_sid, const int* lm_start, bool maps, const int* frame_off, const int* hist_off, const int* hist_label,
                     const int* hist_cnt, int n_frames, int min_kpts, double overlap_ratio, int semantic_matching, int* plan, void* stream) {
    PRAM_REQUIRE(win_sid && win_count && n_win && seg_ids && counts && lm_frame && lm_sel_off && lm_sel_len && (!maps || lm_start) && frame_off &&
                 hist_off && hist_label && hist_cnt && plan, "%s: null pointer", what);
    PRAM_REQUIRE(aligned(win_sid, 4) && aligned(win_count, 4) && aligned(n_win, 4) && aligned(seg_ids, 4) && aligned(counts, 4) &&
                 aligned(lm_frame, 4) && aligned(lm_sel_off, 4) && aligned(lm_sel_len, 4) && aligned(lm_start, 4) && aligned(frame_off, 4) &&
                 aligned(hist_off, 4) && aligned(hist_label, 4) && aligned(hist_cnt, 4) && aligned(plan, 4), "%s: misaligned pointer", what);
    PRAM_REQUIRE(batch >= 0 && batch <= 65535 && n >= 0 && seg_k > 0 && n_class > 0 && n_class <= CAND_MAX_C && n_landmarks >= 0 && n_frames >= 0,
                 "%s: needs 0 <= batch <= 65535, n >= 0, seg_k > 0, 0 < classes <= %d", what, CAND_MAX_C);
    PRAM_REQUIRE((long long)batch * seg_k * (long long)(n > 0 ? n : 1) < 2147483647LL, "%s: batch * seg_k * n does not fit the plan's 32-bit offsets", what);
    PRAM_REQUIRE(overlap_ratio == overlap_ratio && min_kpts >= 0, "%s: overlap_ratio is NaN or min_kpts < 0", what);
    if (batch == 0) return PRAM_OK;
    auto kernel = maps ? cand_plan_kernel<true> : cand_plan_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(seg_k, batch), dim3(256), 0, (hipStream_t)stream, win_sid, win_count, n_win, seg_ids, counts, n, seg_k, lm_frame,
                       lm_sel_off, lm_sel_len, n_landmarks, start_sid, lm_start, n_frames, frame_off, hist_off, hist_label, hist_cnt, min_kpts,
                       overlap_ratio, semantic_matching != 0, plan);
    return pram_launch_status(what);
}

}  // namespace

extern "C" int pram_cand_plan(const int* win_sid, const int* win_count, const int* n_win, const int* seg_ids, const int* counts,
                              int batch, int n, int n_class, int seg_k, const int* lm_frame, const int* lm_sel_off,
                              const int* lm_sel_len, int n_landmarks, int start_sid, const int* frame_off, const int* hist_off,
                              const int* hist_label, const int* hist_cnt, int n_frames, int min_kpts, double overlap_ratio,
                              int semantic_matching, int* plan, void* stream) {
    return cand_plan_launch("pram_cand_plan", win_sid, win_count, n_win, seg_ids, counts, batch, n, n_class, seg_k, lm_frame, lm_sel_off, lm_sel_len,
                            n_landmarks, start_sid, nullptr, false, frame_off, hist_off, hist_label, hist_cnt, n_frames, min_kpts, overlap_ratio,
                            semantic_matching, plan, stream);
}

extern "C" int pram_cand_plan_maps(const int* win_sid, const int* win_count, const int* n_win, const int* seg_ids, const int* counts,
                                   int batch, int n, int n_class, int seg_k, const int* lm_frame, const int* lm_sel_off,
                                   const int* lm_sel_len, int n_landmarks, const int* lm_start, const int* frame_off, const int* hist_off,
                                   const int* hist_label, const int* hist_cnt, int n_frames, int min_kpts, double overlap_ratio,
                                   int semantic_matching, int* plan, void* stream) {
    return cand_plan_launch("pram_cand_plan_maps", win_sid, win_count, n_win, seg_ids, counts, batch, n, n_class, seg_k, lm_frame, lm_sel_off,
                            lm_sel_len, n_landmarks, 0, lm_start, true, frame_off, hist_off, hist_label, hist_cnt, n_frames, min_kpts, overlap_ratio,
                            semantic_matching, plan, stream);
}

extern "C" int pram_cand_gather(const int* plan, const int* tokens, const int* sel_rows, const float* q_desc, const float* q_kpts,
                                const float* q_scores, int n, const float* r_desc, const float* r_kpts, const float* r_scores,
                                const float* frame_norm, int ref_rows, float q_cx, float q_cy, float q_scale, float* desc0, float* nkpts0,
                                float* scores0, float* desc1, float* nkpts1, float* scores1, int pairs, int t_pad, void* stream) {
    PRAM_REQUIRE(plan && tokens && sel_rows && q_desc && q_kpts && q_scores && r_desc && r_kpts && r_scores && frame_norm && desc0 && nkpts0 &&
                 scores0 && desc1 && nkpts1 && scores1, "pram_cand_gather: null pointer");
    PRAM_REQUIRE(aligned(q_desc, 16) && aligned(r_desc, 16) && aligned(desc0, 16) && aligned(desc1, 16),
                 "pram_cand_gather: descriptor buffers must be 16-byte aligned");
    PRAM_REQUIRE(aligned(plan, 4) && aligned(tokens, 4) && aligned(sel_rows, 4) && aligned(q_kpts, 4) && aligned(q_scores, 4) && aligned(r_kpts, 4) &&
                 aligned(r_scores, 4) && aligned(frame_norm, 4) && aligned(nkpts0, 4) && aligned(scores0, 4) && aligned(nkpts1, 4) && aligned(scores1, 4),
                 "pram_cand_gather: misaligned pointer");
    PRAM_REQUIRE(pairs >= 0 && 2 * (long long)pairs <= 65535 && t_pad >= 0 && n >= 0 && ref_rows >= 0 && q_scale > 0.f,
                 "pram_cand_gather: needs 0 <= pairs <= 32767, t_pad >= 0, n >= 0, ref_rows >= 0, q_scale > 0");
    if (pairs == 0 || t_pad == 0) return PRAM_OK;
    hipLaunchKernelGGL(cand_gather_kernel, dim3(cdiv(t_pad, 4), 2 * pairs), dim3(256), 0, (hipStream_t)stream, plan, tokens, sel_rows, q_desc,
                       q_kpts, q_scores, n, r_desc, r_kpts, r_scores, frame_norm, ref_rows, q_cx, q_cy, q_scale, desc0, nkpts0, scores0, desc1,
                       nkpts1, scores1, pairs, t_pad);
    return pram_launch_status("pram_cand_gather");
}

extern "C" int pram_cand_correspond(const long long* matches0, int ldm, const int* plan, const int* tokens, const int* sel_rows,
                                    const float* q_kpts, int n, const float* r_kpts, const double* r_xyz, const long long* r_point3d_ids,
                                    const int* r_segs, int ref_rows, int pairs, int t0, int cap, long long* m_kpt_ids, float* m_kpts,
                                    float* m_ref_kpts, long long* m_point3d_ids, double* m_xyz, int* m_sids, int* m_count, void* stream) {
    PRAM_REQUIRE(matches0 && plan && tokens && sel_rows && q_kpts && r_kpts && r_xyz && r_point3d_ids && r_segs && m_kpt_ids && m_kpts &&
                 m_ref_kpts && m_point3d_ids && m_xyz && m_sids && m_count, "pram_cand_correspond: null pointer");
    PRAM_REQUIRE(aligned(matches0, 8) && aligned(r_xyz, 8) && aligned(r_point3d_ids, 8) && aligned(m_kpt_ids, 8) && aligned(m_point3d_ids, 8) &&
                 aligned(m_xyz, 8), "pram_cand_correspond: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(plan, 4) && aligned(tokens, 4) && aligned(sel_rows, 4) && aligned(q_kpts, 4) && aligned(r_kpts, 4) && aligned(r_segs, 4) &&
                 aligned(m_kpts, 4) && aligned(m_ref_kpts, 4) && aligned(m_sids, 4) && aligned(m_count, 4), "pram_cand_correspond: misaligned pointer");
    PRAM_REQUIRE(pairs >= 0 && t0 >= 0 && ldm >= t0 && cap >= 0 && n >= 0 && ref_rows >= 0,
                 "pram_cand_correspond: needs pairs >= 0, 0 <= t0 <= ldm, cap >= 0, n >= 0, ref_rows >= 0");
    if (pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(cand_correspond_kernel, dim3(pairs), dim3(256), 0, (hipStream_t)stream, matches0, ldm, plan, tokens, sel_rows, q_kpts, n,
                       r_kpts, reinterpret_cast<const long long*>(r_xyz), r_point3d_ids, r_segs, ref_rows, t0, cap,
                       match_list(m_kpt_ids, m_kpts, m_ref_kpts, m_point3d_ids, m_xyz, m_sids), m_count);
    return pram_launch_status("pram_cand_correspond");
}
