// Building blocks the localisation glue kernels share (candidates.hip, refine.hip, projref.hip, track.hip, retrieval.hip,
// extras.hip): the columns of the plan table, the match list and its row copies, the search over the sorted point ids, and the
// covisible list of the frame a localisation kept.  Two of them serve every file that searches or walks a CSR table (kmeans.hip,
// triangulate.hip, twoview.hip, mapper.hip, mapbuild.hip and compress.hip too): the one bisection, first_true, and clamped_range.
// The collectives (ordered compaction, the workgroup's sums and maxima) are workgroup.h's, which every includer gets from here.
#pragma once
#include "workgroup.h"

// column-major plan table: field X of pair p at plan[X * pairs + p]
enum { PL_QUERY = 0, PL_SID, PL_FRAME, PL_SEM, PL_LEN0, PL_LEN1, PL_TOK_OFF, PL_ROW0, PL_SEL_OFF, PL_ORDER };
static_assert(PL_ORDER + 1 == PRAM_CAND_PLAN_COLS, "plan table layout");

// The match list: six parallel arrays, row stride 1, 2, 2, 1, 3 (the bits of float64), 1.  Kernels take it by value; ref_kpts is
// null for a list that carries none (pram_projref_correspond's), which is a property of the launch, not of a row.
struct MatchList { long long* ids; float* kpts; float* ref_kpts; long long* p3d; long long* xyz; int* sids; };
struct ConstMatchList { const long long* ids; const float* kpts; const float* ref_kpts; const long long* p3d; const long long* xyz; const int* sids; };

// the entries' flat pointers -> the struct (xyz: float64 moved as 64-bit words)
static inline MatchList match_list(long long* ids, float* kpts, float* ref_kpts, long long* p3d, double* xyz, int* sids) {
    return {ids, kpts, ref_kpts, p3d, reinterpret_cast<long long*>(xyz), sids};
}
static inline ConstMatchList match_list(const long long* ids, const float* kpts, const float* ref_kpts, const long long* p3d, const double* xyz,
                                        const int* sids) {
    return {ids, kpts, ref_kpts, p3d, reinterpret_cast<const long long*>(xyz), sids};
}

// Both row helpers load the whole row before they store any of it: the struct's members carry no __restrict__, and the loads of
// one row are independent.
// row q of src -> row d of dst
__device__ __forceinline__ void match_copy_row(const MatchList& dst, size_t d, const ConstMatchList& src, size_t q) {
    const long long id = src.ids[q], p3d = src.p3d[q], x = src.xyz[q * 3], y = src.xyz[q * 3 + 1], z = src.xyz[q * 3 + 2];
    const float ku = src.kpts[q * 2], kv = src.kpts[q * 2 + 1], ru = src.ref_kpts[q * 2], rv = src.ref_kpts[q * 2 + 1];
    const int sid = src.sids[q];
    dst.ids[d] = id;
    dst.kpts[d * 2] = ku; dst.kpts[d * 2 + 1] = kv;
    dst.ref_kpts[d * 2] = ru; dst.ref_kpts[d * 2 + 1] = rv;
    dst.p3d[d] = p3d;
    dst.xyz[d * 3] = x; dst.xyz[d * 3 + 1] = y; dst.xyz[d * 3 + 2] = z;
    dst.sids[d] = sid;
}

// keypoint `id` of the query (its coordinates at q_kpt) matched to row rr of a reference side -> row d of dst.  r_kpts is read
// only where dst has ref_kpts.
__device__ __forceinline__ void match_emit_row(const MatchList& dst, size_t d, long long id, const float* __restrict__ q_kpt,
                                               const float* __restrict__ r_kpts, const long long* __restrict__ r_p3d,
                                               const long long* __restrict__ r_xyz, const int* __restrict__ r_sids, size_t rr) {
    const bool with_ref = dst.ref_kpts != nullptr;      // uniform over the kernel
    const long long p3d = r_p3d[rr], x = r_xyz[rr * 3], y = r_xyz[rr * 3 + 1], z = r_xyz[rr * 3 + 2];
    const float ku = q_kpt[0], kv = q_kpt[1], ru = with_ref ? r_kpts[rr * 2] : 0.f, rv = with_ref ? r_kpts[rr * 2 + 1] : 0.f;
    const int sid = r_sids[rr];
    dst.ids[d] = id;
    dst.kpts[d * 2] = ku; dst.kpts[d * 2 + 1] = kv;
    if (with_ref) { dst.ref_kpts[d * 2] = ru; dst.ref_kpts[d * 2 + 1] = rv; }
    dst.p3d[d] = p3d;
    dst.xyz[d * 3] = x; dst.xyz[d * 3 + 1] = y; dst.xyz[d * 3 + 2] = z;
    dst.sids[d] = sid;
}

// The one bisection: the first index i in [lo, hi) at which the monotone predicate holds (false ... false true ... true), hi if
// it holds nowhere; pred is called with indices of [lo, hi) only.  32 steps cover every range an int holds.
template <class Pred>
__device__ __forceinline__ int first_true(int lo, int hi, Pred pred) {
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (pred(mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// first index i of the ascending ids [n] with ids[i] >= id (n if none)
__device__ __forceinline__ int lower_bound_i64(const long long* __restrict__ ids, int n, long long id) {
    return first_true(0, n, [&](int i) { return ids[i] >= id; });
}

// a CSR range (off[i], off[i + 1]) cut into a table of n entries: 0 <= beg <= end <= n, whatever the offsets hold
__device__ __forceinline__ void clamped_range(int o0, int o1, int n, int& beg, int& end) {
    beg = o0 < 0 ? 0 : (o0 > n ? n : o0);
    end = o1 < beg ? beg : (o1 > n ? n : o1);
}

// the frame the localisation kept for query b (-1: not located, disabled, or a frame the store does not hold), and its covisible
// list covis_frames[c0 .. c0 + len) cut to n_cov and to the n_covis entries the table has
struct Slots { int f, c0, len; };

__device__ __forceinline__ Slots query_slots(const int* __restrict__ chosen, const int* __restrict__ loc_plan, const int* __restrict__ enable,
                                             const int* __restrict__ covis_off, int b, int batch, int seg_k, int n_cov, int n_frames,
                                             int n_covis) {
    Slots s = {-1, 0, 0};
    const int kept = chosen[b * 3];
    if (kept >= 0 && kept < seg_k) s.f = loc_plan[(size_t)PL_FRAME * batch * seg_k + b * seg_k + kept];
    if (s.f >= n_frames || (enable != nullptr && enable[b] == 0)) s.f = -1;
    if (s.f < 0) { s.f = -1; return s; }
    s.c0 = covis_off[s.f];
    s.len = covis_off[s.f + 1] - s.c0;
    s.c0 = s.c0 < 0 ? 0 : s.c0;
    s.len = s.len < 0 ? 0 : (s.len > n_cov ? n_cov : s.len);
    if (s.c0 + s.len > n_covis) s.len = n_covis > s.c0 ? n_covis - s.c0 : 0;
    return s;
}
