// Pose refinement by projection over covisible frames (SingleMap3D.refine_pose_by_projection, singlemap3d.py:367-498) for a batch
// of located queries: the union of the points the covisible frames observe (a per-query bitmap over the store's point table),
// their projection with the localisation's pose and the frustum test in float64, the fused range-gated descriptor matching
// (no [M, N] matrix), and the compaction of the accepted keypoints into pram_cand_correspond's layout.  Plain vector loads and
// stores, one idempotent integer atomic (the bitmap's OR), no float atomics; every loop is bounded by an argument and every index
// read from a table is checked against the size given beside it before it is used.  Results do not depend on scheduling.
#include "glue.h"

namespace {

// grid (n_cov + 1, batch): slot j < n_cov = entry j of the list, slot n_cov = the reference frame when the list does not hold it
__global__ __launch_bounds__(256) void projref_mark_kernel(const int* __restrict__ chosen, const int* __restrict__ loc_plan,
                                                           const int* __restrict__ enable, const int* __restrict__ frame_off,
                                                           const int* __restrict__ covis_off, const int* __restrict__ covis_frames,
                                                           const long long* __restrict__ point3d_ids, const long long* __restrict__ pt_ids,
                                                           int batch, int seg_k, int n_cov, int n_frames, int n_covis, int n_rows,
                                                           int n_points, int words, unsigned int* bitmap, int* __restrict__ ref_frame) {
    const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    const Slots s = query_slots(chosen, loc_plan, enable, covis_off, b, batch, seg_k, n_cov, n_frames, n_covis);
    if (j == 0 && tid == 0) ref_frame[b] = s.f;
    if (s.f < 0) return;
    int g = -1;
    if (j < n_cov) {
        if (j < s.len) g = covis_frames[s.c0 + j];
    } else {
        bool in_list = false;
        for (int i = 0; i < s.len; ++i) in_list |= covis_frames[s.c0 + i] == s.f;      // singlemap3d.py:380
        if (!in_list) g = s.f;
    }
    if (g < 0 || g >= n_frames) return;
    int r0 = frame_off[g], r1 = frame_off[g + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > n_rows ? n_rows : r1;
    unsigned int* bits = bitmap + (size_t)b * words;
    for (int r = r0 + tid; r < r1; r += 256) {
        const long long id = point3d_ids[r];
        if (id == -1) continue;
        const int lo = lower_bound_i64(pt_ids, n_points, id);
        if (lo >= n_points || pt_ids[lo] != id) continue;      // a point the table does not hold marks nothing
        atomicOr(&bits[lo >> 5], 1u << (lo & 31));
    }
}

constexpr int PROJ_THREADS = 1024, PROJ_WAVES = PROJ_THREADS / 64;

// one workgroup per query.  Phase 1: the marked points in ascending table index into cand_pt (one bitmap word per thread and
// step).  Phase 2: project, frustum test, ordered compaction in place (a chunk is read, then a barrier, then written at or before
// the positions read so far).
__global__ __launch_bounds__(PROJ_THREADS) void projref_project_kernel(const unsigned int* __restrict__ bitmap, int words, int n_points,
                                                                       const double* __restrict__ pt_xyz, const int* __restrict__ chosen,
                                                                       const double* __restrict__ qvec, const double* __restrict__ tvec,
                                                                       const int* __restrict__ cam_model, const double* __restrict__ cam_params,
                                                                       const int* __restrict__ image_size, int seg_k, int cap,
                                                                       int* cand_pt, double* __restrict__ cand_uv,
                                                                       int* __restrict__ n_union, int* __restrict__ n_cand) {
    __shared__ int wsum[PROJ_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    int* pts = cand_pt + (size_t)b * cap;
    double* uv = cand_uv + (size_t)b * 2 * cap;
    const unsigned int* bits = bitmap + (size_t)b * words;
    int base = 0;
    for (int w0 = 0; w0 < words; w0 += PROJ_THREADS) {
        const int w = w0 + tid;
        unsigned int word = w < words ? bits[w] : 0u;
        if (w == words - 1 && (n_points & 31)) word &= (1u << (n_points & 31)) - 1u;
        int tot;
        int o = base + chunk_offset_n<PROJ_WAVES>(__popc(word), wsum, tot);
        while (word) {
            const int bit = __ffs(word) - 1;
            word &= word - 1u;
            if (o < cap) pts[o] = w * 32 + bit;
            ++o;
        }
        base += tot;
    }
    const int n_u = base < cap ? base : cap;
    __syncthreads();      // phase 2 reads what other threads of this workgroup wrote
    const int kept = chosen[b * 3];
    double R[9], t[3], K[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    double imw = 0.0, imh = 0.0;
    if (n_u > 0 && kept >= 0 && kept < seg_k) {
        const double* q = qvec + (size_t)(b * seg_k + kept) * 4;
        const double* tv = tvec + (size_t)(b * seg_k + kept) * 3;
        const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        // qvec2rotmat (colmap_utils/read_write_model.py:556-566), its operation order
        R[0] = (1.0 - (2.0 * (q2 * q2))) - (2.0 * (q3 * q3)); R[1] = ((2.0 * q1) * q2) - ((2.0 * q0) * q3); R[2] = ((2.0 * q3) * q1) + ((2.0 * q0) * q2);
        R[3] = ((2.0 * q1) * q2) + ((2.0 * q0) * q3); R[4] = (1.0 - (2.0 * (q1 * q1))) - (2.0 * (q3 * q3)); R[5] = ((2.0 * q2) * q3) - ((2.0 * q0) * q1);
        R[6] = ((2.0 * q3) * q1) - ((2.0 * q0) * q2); R[7] = ((2.0 * q2) * q3) + ((2.0 * q0) * q1); R[8] = (1.0 - (2.0 * (q1 * q1))) - (2.0 * (q2 * q2));
        t[0] = tv[0]; t[1] = tv[1]; t[2] = tv[2];
        const double* cp = cam_params + (size_t)b * PRAM_POSE_CAM_PARAMS;
        const int model = cam_model[b];
        // Frame.get_intrinsics (localization/frame.py:154-175): one focal length for SIMPLE_PINHOLE, SIMPLE_RADIAL, RADIAL
        if (model == PRAM_CAM_PINHOLE || model == PRAM_CAM_OPENCV) { K[0] = cp[0]; K[4] = cp[1]; K[2] = cp[2]; K[5] = cp[3]; }
        else { K[0] = cp[0]; K[4] = cp[0]; K[2] = cp[1]; K[5] = cp[2]; }
        imw = (double)image_size[b * 2];
        imh = (double)image_size[b * 2 + 1];
    }
    const int n_p = (kept >= 0 && kept < seg_k) ? n_u : 0;      // marks exist only for a located query
    base = 0;
    for (int c0 = 0; c0 < n_p; c0 += PROJ_THREADS) {
        const int i = c0 + tid;
        int pt = -1;
        double u = 0.0, v = 0.0;
        bool keep = false;
        if (i < n_p) {
            pt = pts[i];
            const double x = pt_xyz[(size_t)pt * 3], y = pt_xyz[(size_t)pt * 3 + 1], z = pt_xyz[(size_t)pt * 3 + 2];
            double c[3], p[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) c[r] = ((R[r * 3] * x + R[r * 3 + 1] * y) + R[r * 3 + 2] * z) + t[r];      // pram_project_points_f64's order
#pragma unroll
            for (int r = 0; r < 3; ++r) p[r] = (K[r * 3] * c[0] + K[r * 3 + 1] * c[1]) + K[r * 3 + 2] * c[2];
            u = p[0] / p[2];
            v = p[1] / p[2];
            keep = (p[2] > 0.0) && (p[2] < 100.0) && (u >= 0.0) && (u < imw) && (v >= 0.0) && (v < imh);
        }
        int tot;
        const int o = base + chunk_offset<PROJ_WAVES>(keep, wsum, tot);      // its barriers stand between the chunk's reads and writes
        if (keep) {
            pts[o] = pt;
            uv[o] = u;
            uv[cap + o] = v;
        }
        base += tot;
    }
    if (tid == 0) { n_union[b] = n_u; n_cand[b] = base; }
}

// one wave per (query, keypoint).  Lanes stride over the candidates for the range test; for every in-range candidate, ascending,
// the wave reads the point's descriptor row (lane l: elements 2l, 2l + 1), and
//     sim = butterfly over lanes (xor 32, 16, 8, 4, 2, 1) of  (q[2l] * r[2l]) + (q[2l + 1] * r[2l + 1])
// which leaves the same bits in every lane (fp32 addition commutes); that is the ONE reduction order.
__global__ __launch_bounds__(256) void projref_match_kernel(const float* __restrict__ q_kpts, const float* __restrict__ q_desc,
                                                            const int* __restrict__ counts, int n, const int* __restrict__ cand_pt,
                                                            const double* __restrict__ cand_uv, const int* __restrict__ n_cand, int cap,
                                                            const float* __restrict__ pt_desc, int n_points, double range,
                                                            int* __restrict__ best, float* __restrict__ d0, float* __restrict__ d1,
                                                            unsigned char* __restrict__ accept) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const size_t row = (size_t)b * n + i;
    int nq = counts[b], nc = n_cand[b];
    nq = nq > n ? n : nq;
    nc = nc < 0 ? 0 : (nc > cap ? cap : nc);
    float a0 = INFINITY, a1 = INFINITY;
    int j0 = -1, n_in = 0;
    if (i < nq) {
        const double kx = (double)q_kpts[row * 2], ky = (double)q_kpts[row * 2 + 1];
        const float2 q = reinterpret_cast<const float2*>(q_desc + row * 128)[lane];
        const int* pts = cand_pt + (size_t)b * cap;
        const double* uv = cand_uv + (size_t)b * 2 * cap;
        // sqrt is monotone and correctly rounded: a squared error outside [lo, hi] decides the test without it
        const double r2 = range * range, lo = r2 * (1.0 - 1e-12), hi = r2 * (1.0 + 1e-12);
        for (int c0 = 0; c0 < nc; c0 += 64) {
            const int c = c0 + lane;
            bool in = false;
            int pt = -1;
            if (c < nc) {
                const double ex = kx - uv[c], ey = ky - uv[cap + c];
                const double s = ex * ex + ey * ey;
                in = s < lo ? true : (s > hi ? false : !(sqrt(s) >= range));      // in range = NOT (error >= 2 * threshold), singlemap3d.py:426
                if (in) pt = pts[c];
            }
            unsigned long long hits = __ballot(in);
            while (hits) {
                const int l = __ffsll((long long)hits) - 1;
                hits &= hits - 1ull;
                const int p = __shfl(pt, l, 64);
                ++n_in;
                if (p < 0 || p >= n_points) continue;      // never true for pram_projref_project's output
                const float2 r = reinterpret_cast<const float2*>(pt_desc + (size_t)p * 128)[lane];
                float sim = (q.x * r.x) + (q.y * r.y);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) sim += __shfl_xor(sim, o, 64);
                const float d = sqrtf((2.f - 2.f * sim) + 1e-6f);
                if (d < a0) { a1 = a0; a0 = d; j0 = c0 + l; }
                else if (d < a1) a1 = d;
            }
        }
    }
    if (lane == 0) {
        best[row] = j0;
        d0[row] = a0;
        d1[row] = a1;
        // topk(k = 2) needs two candidates; one in range: the second distance carries + 100 and the ratio passes
        accept[row] = (nc >= 2 && j0 >= 0 && (n_in == 1 || a0 / a1 <= 0.995f)) ? 1 : 0;
    }
}

// one workgroup per query: ballot + prefix compaction of accept in ascending keypoint index
__global__ __launch_bounds__(256) void projref_correspond_kernel(const unsigned char* __restrict__ accept, const int* __restrict__ best,
                                                                 const int* __restrict__ counts, const float* __restrict__ q_kpts, int n,
                                                                 const int* __restrict__ cand_pt, const int* __restrict__ n_cand, int cap,
                                                                 const long long* __restrict__ pt_ids, const long long* __restrict__ pt_xyz,
                                                                 const int* __restrict__ pt_sid, int n_points, MatchList m,
                                                                 int* __restrict__ m_count) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int nq = counts[b], nc = n_cand[b];
    nq = nq < 0 ? 0 : (nq > n ? n : nq);
    nc = nc < 0 ? 0 : (nc > cap ? cap : nc);
    int base = 0;
    for (int i0 = 0; i0 < nq; i0 += 256) {
        const int i = i0 + tid;
        const size_t row = (size_t)b * n + i;
        int pt = -1;
        if (i < nq && accept[row]) {
            const int j = best[row];
            if (j >= 0 && j < nc) pt = cand_pt[(size_t)b * cap + j];
            if (pt >= n_points) pt = -1;
        }
        int tot;
        const int o = base + chunk_offset<4>(pt >= 0, wsum, tot);
        // the list has no ref_kpts (a point of the map has no keypoint of its own), so the helper reads no reference keypoints
        if (pt >= 0) match_emit_row(m, (size_t)b * n + o, i, q_kpts + row * 2, nullptr, pt_ids, pt_xyz, pt_sid, (size_t)pt);
        base += tot;
    }
    if (tid == 0) m_count[b] = base;
}

}  // namespace

extern "C" int pram_projref_mark(const int* chosen, const int* loc_plan, const int* enable, const int* frame_off, const int* covis_off,
                                 const int* covis_frames, const long long* point3d_ids, const long long* pt_ids, int batch, int seg_k,
                                 int n_cov, int n_frames, int n_covis, int n_rows, int n_points, unsigned int* bitmap, int* ref_frame,
                                 void* stream) {
    PRAM_REQUIRE(chosen && loc_plan && frame_off && covis_off && covis_frames && point3d_ids && pt_ids && bitmap && ref_frame,
                 "pram_projref_mark: null pointer");
    PRAM_REQUIRE(aligned(point3d_ids, 8) && aligned(pt_ids, 8), "pram_projref_mark: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(chosen, 4) && aligned(loc_plan, 4) && aligned(enable, 4) && aligned(frame_off, 4) && aligned(covis_off, 4) &&
                 aligned(covis_frames, 4) && aligned(bitmap, 4) && aligned(ref_frame, 4), "pram_projref_mark: misaligned pointer");
    PRAM_REQUIRE(n_cov > 0 && n_cov < 65535, "pram_projref_mark: needs 0 < n_cov < 65535");
    PRAM_REQUIRE(batch >= 0 && batch <= 65535 && seg_k >= 1 && n_frames >= 0 && n_covis >= 0 && n_rows >= 0 && n_points >= 1,
                 "pram_projref_mark: needs 0 <= batch <= 65535, seg_k >= 1, n_frames >= 0, n_covis >= 0, n_rows >= 0, n_points >= 1");
    PRAM_REQUIRE((long long)batch * seg_k < 2147483647LL / PRAM_CAND_PLAN_COLS, "pram_projref_mark: batch * seg_k does not fit the plan's 32-bit offsets");
    if (batch == 0) return PRAM_OK;
    const int words = cdiv(n_points, 32);
    if (hipMemsetD32Async((hipDeviceptr_t)bitmap, 0, (size_t)batch * words, (hipStream_t)stream) != hipSuccess)
        return pram_launch_status("pram_projref_mark");
    hipLaunchKernelGGL(projref_mark_kernel, dim3(n_cov + 1, batch), dim3(256), 0, (hipStream_t)stream, chosen, loc_plan, enable, frame_off,
                       covis_off, covis_frames, point3d_ids, pt_ids, batch, seg_k, n_cov, n_frames, n_covis, n_rows, n_points, words, bitmap,
                       ref_frame);
    return pram_launch_status("pram_projref_mark");
}

extern "C" int pram_projref_project(const unsigned int* bitmap, int n_points, const double* pt_xyz, const int* chosen, const double* qvec,
                                    const double* tvec, const int* cam_model, const double* cam_params, const int* image_size, int batch,
                                    int seg_k, int cap, int* cand_pt, double* cand_uv, int* n_union, int* n_cand, void* stream) {
    PRAM_REQUIRE(bitmap && pt_xyz && chosen && qvec && tvec && cam_model && cam_params && image_size && cand_pt && cand_uv && n_union && n_cand,
                 "pram_projref_project: null pointer");
    PRAM_REQUIRE(aligned(pt_xyz, 8) && aligned(qvec, 8) && aligned(tvec, 8) && aligned(cam_params, 8) && aligned(cand_uv, 8),
                 "pram_projref_project: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(bitmap, 4) && aligned(chosen, 4) && aligned(cam_model, 4) && aligned(image_size, 4) && aligned(cand_pt, 4) &&
                 aligned(n_union, 4) && aligned(n_cand, 4), "pram_projref_project: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && seg_k >= 1 && n_points >= 1 && cap >= 1, "pram_projref_project: needs batch >= 0, seg_k >= 1, n_points >= 1, cap >= 1");
    PRAM_REQUIRE((long long)batch * seg_k < 2147483647LL, "pram_projref_project: batch * seg_k overflows");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(projref_project_kernel, dim3(batch), dim3(PROJ_THREADS), 0, (hipStream_t)stream, bitmap, cdiv(n_points, 32), n_points, pt_xyz,
                       chosen, qvec, tvec, cam_model, cam_params, image_size, seg_k, cap, cand_pt, cand_uv, n_union, n_cand);
    return pram_launch_status("pram_projref_project");
}

extern "C" int pram_projref_match(const float* q_kpts, const float* q_desc, const int* counts, int batch, int n, const int* cand_pt,
                                  const double* cand_uv, const int* n_cand, int cap, const float* pt_desc, int n_points, double threshold,
                                  int* best, float* d0, float* d1, unsigned char* accept, void* stream) {
    PRAM_REQUIRE(q_kpts && q_desc && counts && cand_pt && cand_uv && n_cand && pt_desc && best && d0 && d1 && accept,
                 "pram_projref_match: null pointer");
    PRAM_REQUIRE(aligned(cand_uv, 8) && aligned(q_desc, 8) && aligned(pt_desc, 8), "pram_projref_match: cand_uv and the descriptors must be 8-byte aligned");
    PRAM_REQUIRE(aligned(q_kpts, 4) && aligned(counts, 4) && aligned(cand_pt, 4) && aligned(n_cand, 4) && aligned(best, 4) && aligned(d0, 4) &&
                 aligned(d1, 4), "pram_projref_match: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && batch <= 65535 && n >= 0 && n_points >= 1 && cap >= 1, "pram_projref_match: needs 0 <= batch <= 65535, n >= 0, n_points >= 1, cap >= 1");
    PRAM_REQUIRE(threshold > 0.0 && threshold < 1e150, "pram_projref_match: needs a finite threshold > 0");
    if (batch == 0 || n == 0) return PRAM_OK;
    hipLaunchKernelGGL(projref_match_kernel, dim3(cdiv(n, 4), batch), dim3(256), 0, (hipStream_t)stream, q_kpts, q_desc, counts, n, cand_pt, cand_uv,
                       n_cand, cap, pt_desc, n_points, 2.0 * threshold, best, d0, d1, accept);
    return pram_launch_status("pram_projref_match");
}

extern "C" int pram_projref_correspond(const unsigned char* accept, const int* best, const int* counts, const float* q_kpts, int batch, int n,
                                       const int* cand_pt, const int* n_cand, int cap, const long long* pt_ids, const double* pt_xyz,
                                       const int* pt_sid, int n_points, long long* m_kpt_ids, float* m_kpts, long long* m_point3d_ids,
                                       double* m_xyz, int* m_sids, int* m_count, void* stream) {
    PRAM_REQUIRE(accept && best && counts && q_kpts && cand_pt && n_cand && pt_ids && pt_xyz && pt_sid && m_kpt_ids && m_kpts && m_point3d_ids &&
                 m_xyz && m_sids && m_count, "pram_projref_correspond: null pointer");
    PRAM_REQUIRE(aligned(pt_ids, 8) && aligned(pt_xyz, 8) && aligned(m_kpt_ids, 8) && aligned(m_point3d_ids, 8) && aligned(m_xyz, 8),
                 "pram_projref_correspond: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(best, 4) && aligned(counts, 4) && aligned(q_kpts, 4) && aligned(cand_pt, 4) && aligned(n_cand, 4) && aligned(pt_sid, 4) &&
                 aligned(m_kpts, 4) && aligned(m_sids, 4) && aligned(m_count, 4), "pram_projref_correspond: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && n >= 0 && n_points >= 1 && cap >= 1, "pram_projref_correspond: needs batch >= 0, n >= 0, n_points >= 1, cap >= 1");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(projref_correspond_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, accept, best, counts, q_kpts, n, cand_pt, n_cand,
                       cap, pt_ids, reinterpret_cast<const long long*>(pt_xyz), pt_sid, n_points,
                       match_list(m_kpt_ids, m_kpts, nullptr, m_point3d_ids, m_xyz, m_sids), m_count);
    return pram_launch_status("pram_projref_correspond");
}
