// Global bundle adjustment of a map on the device: the frames' poses (cam_from_world) and the points, jointly, under the robust
// cost of pose.hip (s = |r|^2 / loss_scale^2, cost log1p(s), weight 1 / (1 + s)), intrinsics constant (pram_ba_*) or, per camera
// group, refined with them (pram_bac_*: the struct Bac below).  Levenberg-Marquardt; the
// reduced camera system S d_c = b of the Schur complement is solved by matrix-free conjugate gradients with the block-Jacobi
// preconditioner; the stop tests, alpha, beta, the accept / reject decision and lam live in a state record on the device that
// every kernel reads, so nothing is read by the host inside a solve and a finished solve turns the launches that are still
// enqueued into early exits.  float64 throughout, no floating-point atomics; every sum has one fixed order:
//   * per point over its observations: per lane in ascending order, then the butterfly of wave_sum_f64 (one wave per point);
//   * per frame over its observations: the same per wave, then the fixed 4-wave fold of block_fold_f64 (one workgroup);
//   * over frames (dot products, the cost): blocks of PRAM_BA_BLOCK consecutive frames added to 0.0 in ascending order, the block
//     partials added to 0.0 in ascending order (the blocked order of kmeans.hip).
// The final filter is COLMAP's point filter (FilterPoints3D: reprojection error and the largest triangulation angle) as
// understood from its source.  pycolmap is not installed and was never run beside this, so nothing here is pinned to it.
#include "obs.h"
#include "ransac.h"
#include "glue.h"
#include <math.h>
#include <string.h>

namespace {

__device__ __forceinline__ int cdiv_d(int a, int b) { return (a + b - 1) / b; }

constexpr int JW = PRAM_BA_OBS_DOUBLES;      // per observation: sqrt(w) J_c [2][6], sqrt(w) J_p [2][3], sqrt(w) r [2]
constexpr int BLK = PRAM_BA_BLOCK;
constexpr int NV_FRAME = 39;                 // 21 of S's diagonal block without damping, 6 of diag U, 6 of g_c, 6 of W V^-1 g_p

enum { SD_COST = 0, SD_CAND, SD_LAM, SD_RZ, SD_PAP, SD_ALPHA, SD_BETA, SD_BB, SD_RR, SD_COST0, SD_LOSS2, SD_CGTOL, SD_FTOL };
enum { SI_DONE = 0, SI_REASON, SI_LM_ITER, SI_ACCEPTED, SI_CG_ITER, SI_CG_DONE, SI_RELIN, SI_BAD, SI_PENDING, SI_CG_FAIL, SI_MAX_ITERS };
static_assert(SD_FTOL < PRAM_BA_STATE_F64 && SI_MAX_ITERS < PRAM_BA_STATE_I32, "state record layout");
static_assert(SD_COST == PRAM_BA_SD_COST && SD_LAM == PRAM_BA_SD_LAM && SD_COST0 == PRAM_BA_SD_COST0 && SI_DONE == PRAM_BA_SI_DONE &&
              SI_REASON == PRAM_BA_SI_REASON && SI_LM_ITER == PRAM_BA_SI_LM_ITER && SI_ACCEPTED == PRAM_BA_SI_ACCEPTED &&
              SI_CG_FAIL == PRAM_BA_SI_CG_FAIL, "state record layout");

enum { A_T = 0, A_TC, A_X, A_XC, A_J, A_VINV, A_GP, A_YP, A_SBLK, A_DU, A_B, A_CGX, A_CGR, A_CGZ, A_CGP, A_CGQ, A_FDOT, A_FCOST, A_PART, A_SD,
       A_SI, A_PFLAG, A_MOVED, A_FMASK, A_OOK, A_COUNT };
static_assert(A_COUNT == PRAM_BA_ARRAYS, "workspace layout");

struct Ba {
    static constexpr int JW = PRAM_BA_OBS_DOUBLES;
    static constexpr bool CAM = false;
    const float* kpts; const int* cam_model; const double* cam_params;
    const int *obs_row, *obs_frame, *obs_point, *frm_off, *pt_off, *pt_obs, *frozen;
    int F, P, n_obs, n_rows, max_iters;
    double *T, *Tc, *X, *Xc, *J, *Vinv, *gp, *yp, *Sblk, *dU, *b, *x, *r, *z, *p, *q, *fdot, *fcost, *part, *sd;
    int *si, *pflag, *moved, *fmask;
    unsigned char* ook;
    unsigned long long magic;
};
static_assert(sizeof(Ba) <= PRAM_BA_CONTEXT_BYTES, "context size");
constexpr unsigned long long MAGIC = 0x42414354584d4150ull;

// The adjustment that also refines the intrinsics of camera groups: the same problem with 8 further columns per
// observation (sqrt(w) J_k, between J_c and J_p) and 8 further unknowns per group behind the 6 F of the poses.  The base's
// cam_params points at `cp`, the per-frame parameters bac_expand_kernel writes from the groups' accepted parameters, so every
// kernel that takes a Ba runs on this problem unchanged.
constexpr int NK = PRAM_BAC_GROUP_PARAMS;      // a group's parameters: the model's own, COLMAP's order, zero padded
constexpr int NV_GROUP = 60;                   // 36 of the group's block without damping, 8 of diag U_k, 8 of g_k, 8 of W_k V^-1 g_p
static_assert(NK == PRAM_POSE_CAM_PARAMS && PRAM_BAC_OBS_DOUBLES == PRAM_BA_OBS_DOUBLES + 2 * NK, "row layout");

enum { C_CP = A_COUNT, C_CPC, C_K, C_KC, C_SG, C_DUG, C_BG, C_GX, C_GR, C_GZ, C_GP, C_GQ, C_GDOT, C_GPART, C_FPART, C_MVPART, C_GMASK, C_GBAD,
       C_GMODEL, C_GFOLD, C_COUNT };
static_assert(C_COUNT == PRAM_BAC_ARRAYS, "workspace layout");

struct Bac : Ba {
    static constexpr int JW = PRAM_BAC_OBS_DOUBLES;
    static constexpr bool CAM = true;
    const int *frm_grp, *grp_off, *grp_frame, *grp_mask_in;
    const double* grp_params_in;
    int G;
    double *cp, *cpc, *k, *kc, *Sg, *dUg, *bg, *gx, *gr, *gz, *gpv, *gq, *gdot, *gpart, *fpart, *mvpart, *gfold;
    int *gmask, *gbad, *gmodel;
};
static_assert(sizeof(Bac) <= PRAM_BAC_CONTEXT_BYTES, "context size");
constexpr unsigned long long MAGIC_CAM = 0x42414343414d4552ull;

__device__ __forceinline__ Obs obs_view(const Ba& g, const double* table) {
    return {nullptr, g.kpts, table, g.cam_model, g.cam_params, g.F, g.n_rows};
}

// ---------------------------------------------------------------- sums over frames: the blocked fixed order, one workgroup of 256
__device__ double blocked_sum(const double* v, int n, double* part, double* sh) {
    const int tid = threadIdx.x, nb = cdiv_d(n, BLK);
    for (int b = tid; b < nb; b += 256) {
        const int e = (b + 1) * BLK < n ? (b + 1) * BLK : n;
        double s = 0.0;
        for (int i = b * BLK; i < e; ++i) s += v[i];
        part[b] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += part[b];
        sh[0] = s;
    }
    __syncthreads();
    const double out = sh[0];
    __syncthreads();
    return out;
}

// M z = r with the frame's block of S (damped already); a block that does not factor leaves z = r
__device__ __forceinline__ void precond(const double* __restrict__ S, const double* r, double* z) {
    double neg[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) neg[a] = -r[a];
    if (!chol_solve6(S, neg, 0.0, z)) {
#pragma unroll
        for (int a = 0; a < 6; ++a) z[a] = r[a];
    }
}

// ---------------------------------------------------------------- begin: the state record, the tables' check, the frozen masks
__global__ void ba_init_kernel(Ba g, double loss_scale, double lam0, double cg_tol, double ftol) {
    for (int i = 0; i < PRAM_BA_STATE_F64; ++i) g.sd[i] = 0.0;
    for (int i = 0; i < PRAM_BA_STATE_I32 + 2 * g.max_iters; ++i) g.si[i] = 0;
    g.sd[SD_LAM] = lam0; g.sd[SD_LOSS2] = loss_scale * loss_scale; g.sd[SD_CGTOL] = cg_tol; g.sd[SD_FTOL] = ftol;
    g.si[SI_RELIN] = 1; g.si[SI_MAX_ITERS] = g.max_iters;
}

__device__ __forceinline__ void ba_bad(const Ba& g) { g.si[SI_BAD] = 1; g.si[SI_DONE] = 1; g.si[SI_REASON] = PRAM_BA_REASON_TABLES; }

// every index any later kernel dereferences, once: a table that fails ends the run before anything reads through it
__global__ __launch_bounds__(256) void ba_check_kernel(Ba g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && (g.frm_off[0] != 0 || g.frm_off[g.F] != g.n_obs || g.pt_off[0] != 0 || g.pt_off[g.P] != g.n_obs)) ba_bad(g);
    if (i < g.F) {
        const int a = g.frm_off[i], b = g.frm_off[i + 1];
        if (a < 0 || b < a || b > g.n_obs) ba_bad(g);
        g.fmask[i] = b > a ? (g.frozen[i] & 63) : 63;      // a frame without observations does not move
        g.moved[i] = 0;
    }
    if (i < g.P) {
        const int a = g.pt_off[i], b = g.pt_off[i + 1];
        if (a < 0 || b < a || b > g.n_obs) ba_bad(g);
        g.pflag[i] = 1;
    }
    if (i < g.n_obs) {
        const int row = g.obs_row[i], f = g.obs_frame[i], p = g.obs_point[i], o = g.pt_obs[i];
        bool ok = row >= 0 && row < g.n_rows && f >= 0 && f < g.F && p >= 0 && p < g.P && o >= 0 && o < g.n_obs;
        if (ok) {
            const int fa = g.frm_off[f], fb = g.frm_off[f + 1];
            ok = i >= fa && i < fb;
            // position i of the point-major table belongs to the point q with pt_off[q] <= i < pt_off[q + 1]
            const int q = first_true(0, g.P - 1, [&](int k) { return g.pt_off[k + 1] > i; });
            const int po = g.obs_point[o];
            ok = ok && po == q;
        }
        if (!ok) ba_bad(g);
    }
}

__global__ __launch_bounds__(256) void ba_copy_kernel(const double* __restrict__ a, double* __restrict__ o, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) o[i] = a[i];
}

// ---------------------------------------------------------------- linearise: one thread per observation
template <class G>
__global__ __launch_bounds__(256) void ba_linearise_kernel(G g) {
    constexpr int JW = G::JW, OP = G::JW - 8, OR = G::JW - 2;      // J_p and r close the row
    if (g.si[SI_DONE] || !g.si[SI_RELIN]) return;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= g.n_obs) return;
    const int f = g.obs_frame[o], p = g.obs_point[o];
    const double* T = g.T + (size_t)f * FC;
    const V3 X = {g.X[(size_t)p * 3], g.X[(size_t)p * 3 + 1], g.X[(size_t)p * 3 + 2]};
    double z, r0, r1, Jp[6];
    obs_residual(obs_view(g, g.T), g.obs_row[o], f, X, z, r0, r1, true, Jp);
    const double s = (r0 * r0 + r1 * r1) / g.sd[SD_LOSS2];
    const bool ok = z > 1e-12 && fin(s);
    double* out = g.J + (size_t)o * JW;
    g.ook[o] = ok;
    if (!ok) {
#pragma unroll
        for (int e = 0; e < JW; ++e) out[e] = 0.0;
        return;
    }
    const double sw = sqrt(1.0 / (1.0 + s));
    // obs_residual's J_p is A R with A = d residual / d (camera point): A = J_p R^T, and d (camera point) / d (w, d) = (-[Y]x, I)
    const double Y0 = T[0] * X.x + T[1] * X.y + T[2] * X.z, Y1 = T[3] * X.x + T[4] * X.y + T[5] * X.z, Y2 = T[6] * X.x + T[7] * X.y + T[8] * X.z;
    const int mask = g.fmask[f];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double* jp = Jp + i * 3;
        const double a0 = jp[0] * T[0] + jp[1] * T[1] + jp[2] * T[2], a1 = jp[0] * T[3] + jp[1] * T[4] + jp[2] * T[5],
                     a2 = jp[0] * T[6] + jp[1] * T[7] + jp[2] * T[8];
        const double jc[6] = {a2 * Y1 - a1 * Y2, a0 * Y2 - a2 * Y0, a1 * Y0 - a0 * Y1, a0, a1, a2};
#pragma unroll
        for (int a = 0; a < 6; ++a) out[i * 6 + a] = ((mask >> a) & 1) ? 0.0 : sw * jc[a];
#pragma unroll
        for (int k = 0; k < 3; ++k) out[OP + i * 3 + k] = sw * jp[k];
    }
    out[OR] = sw * r0; out[OR + 1] = sw * r1;
    if constexpr (G::CAM) {
        // obs_residual's u, v once more, for the columns of the group's parameters
        const int model = g.cam_model[f];
        const Cam c = cam_unify(model, g.cam_params + (size_t)f * PRAM_POSE_CAM_PARAMS);
        const double u = (Y0 + T[9]) / z, v = (Y1 + T[10]) / z;
        double ud, vd, Jk[2 * NK];
        distort(c, u, v, ud, vd);
        cam_param_jac(model, c, u, v, ud, vd, u * u + v * v, Jk);
        const int km = g.gmask[g.frm_grp[f]];
#pragma unroll
        for (int e = 0; e < 2 * NK; ++e) out[12 + e] = ((km >> (e % NK)) & 1) ? 0.0 : sw * Jk[e];
    }
}

// ---------------------------------------------------------------- blocks
// one wave per point: V = sum J_p^T J_p, g_p, the inverse of V + lam diag(V) by chol_solve3
template <class G>
__global__ __launch_bounds__(64) void ba_points_kernel(G g) {
    constexpr int JW = G::JW;
    if (g.si[SI_DONE]) return;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int beg = g.pt_off[p], end = g.pt_off[p + 1];
    double acc[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = 0.0;
    int cnt = 0;
    for (int k = beg + lane; k < end; k += 64) {
        const int o = g.pt_obs[k];
        const double* j = g.J + (size_t)o * JW + (JW - 8);
        const double r0 = j[6], r1 = j[7];
        cnt += g.ook[o];
        acc[0] += j[0] * j[0] + j[3] * j[3]; acc[1] += j[0] * j[1] + j[3] * j[4]; acc[2] += j[0] * j[2] + j[3] * j[5];
        acc[3] += j[1] * j[1] + j[4] * j[4]; acc[4] += j[1] * j[2] + j[4] * j[5]; acc[5] += j[2] * j[2] + j[5] * j[5];
        acc[6] += j[0] * r0 + j[3] * r1; acc[7] += j[1] * r0 + j[4] * r1; acc[8] += j[2] * r0 + j[5] * r1;
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = wave_sum_f64(acc[e]);
    cnt = wave_sum_i32(cnt);
    if (lane != 0) return;
    const double lam = g.sd[SD_LAM];
    const double A[6] = {acc[0] + lam * acc[0], acc[1], acc[2], acc[3] + lam * acc[3], acc[4], acc[5] + lam * acc[5]};
    const double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
    double c0[3], c1[3], c2[3];
    const bool ok = cnt >= 2 && chol_solve3(A, e0, c0) && chol_solve3(A, e1, c1) && chol_solve3(A, e2, c2);
    double* V = g.Vinv + (size_t)p * 6;
    if (ok) { V[0] = c0[0]; V[1] = c0[1]; V[2] = c0[2]; V[3] = c1[1]; V[4] = c1[2]; V[5] = c2[2]; }
    else { V[0] = 0.0; V[1] = 0.0; V[2] = 0.0; V[3] = 0.0; V[4] = 0.0; V[5] = 0.0; }      // the point stays where it is
    g.pflag[p] = ok;
    g.gp[(size_t)p * 3] = acc[6]; g.gp[(size_t)p * 3 + 1] = acc[7]; g.gp[(size_t)p * 3 + 2] = acc[8];
}

// V^-1 (symmetric, 6 values) times a 3-vector
__device__ __forceinline__ void vinv_mul(const double* __restrict__ V, const double* a, double* o) {
    o[0] = V[0] * a[0] + V[1] * a[1] + V[2] * a[2];
    o[1] = V[1] * a[0] + V[3] * a[1] + V[4] * a[2];
    o[2] = V[2] * a[0] + V[4] * a[1] + V[5] * a[2];
}

// A frame's sums for N parameters whose columns stand at OFF of the row (the pose: 6 at 0; the group's parameters: 8 at 12):
// N (N + 1) / 2 of the diagonal block U - W V^-1 W^T without damping, N of diag U, N of J^T r, N of W V^-1 g_p.
template <class G, int N, int OFF>
__device__ __forceinline__ void frame_terms(const G& g, int beg, int end, int tid, double* acc) {
    constexpr int JW = G::JW, NB = N * (N + 1) / 2;
    for (int o = beg + tid; o < end; o += 256) {
        const double* j = g.J + (size_t)o * JW;
        const int p = g.obs_point[o];
        const double* V = g.Vinv + (size_t)p * 6;
        const double* gp = g.gp + (size_t)p * 3;
        double jc[2 * N], jp[6];
#pragma unroll
        for (int e = 0; e < 2 * N; ++e) jc[e] = j[OFF + e];
#pragma unroll
        for (int e = 0; e < 6; ++e) jp[e] = j[JW - 8 + e];
        const double r0 = j[JW - 2], r1 = j[JW - 1];
        double W[N][3], WV[N][3];
#pragma unroll
        for (int a = 0; a < N; ++a) {
#pragma unroll
            for (int k = 0; k < 3; ++k) W[a][k] = jc[a] * jp[k] + jc[N + a] * jp[3 + k];
            vinv_mul(V, W[a], WV[a]);
        }
        int e = 0;
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int c = a; c < N; ++c) {
                const double u = jc[a] * jc[c] + jc[N + a] * jc[N + c];
                const double w = WV[a][0] * W[c][0] + WV[a][1] * W[c][1] + WV[a][2] * W[c][2];
                acc[e++] += u - w;
            }
#pragma unroll
        for (int a = 0; a < N; ++a) {
            acc[NB + a] += jc[a] * jc[a] + jc[N + a] * jc[N + a];
            acc[NB + N + a] += jc[a] * r0 + jc[N + a] * r1;
            acc[NB + 2 * N + a] += WV[a][0] * gp[0] + WV[a][1] * gp[1] + WV[a][2] * gp[2];
        }
    }
}

// one workgroup per frame: U, g_c, the frame's diagonal block of S = U - W V^-1 W^T and b = W V^-1 g_p - g_c
template <class G>
__global__ __launch_bounds__(256) void ba_frames_kernel(G g) {
    __shared__ double wred[4][NV_FRAME], tot[NV_FRAME];
    if (g.si[SI_DONE]) return;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int beg = g.frm_off[f], end = g.frm_off[f + 1];
    double acc[NV_FRAME];
#pragma unroll
    for (int e = 0; e < NV_FRAME; ++e) acc[e] = 0.0;
    frame_terms<G, 6, 0>(g, beg, end, tid, acc);
    block_fold_f64<NV_FRAME>(acc, wred, tot);
    if (tid != 0) return;
    const double lam = g.sd[SD_LAM];
    const int mask = g.fmask[f];
    double* S = g.Sblk + (size_t)f * 21;
    int e = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) {
            double v = tot[e];
            if (a == c) v = ((mask >> a) & 1) ? 1.0 : v + lam * tot[21 + a];      // a frozen parameter: unit diagonal
            S[e++] = v;
        }
    for (int a = 0; a < 6; ++a) {
        g.dU[(size_t)f * 6 + a] = tot[21 + a];
        g.b[(size_t)f * 6 + a] = tot[33 + a] - tot[27 + a];
    }
}

// one workgroup per frame, a second pass over its observations: the frame's share of its group's sums (NV_GROUP values).  A pass
// of its own, so that neither this kernel nor ba_frames_kernel carries the accumulators of both
__global__ __launch_bounds__(256) void bac_frames_kernel(Bac g) {
    __shared__ double wred[4][NV_GROUP], tot[NV_GROUP];
    if (g.si[SI_DONE]) return;
    const int f = blockIdx.x, tid = threadIdx.x;
    double acc[NV_GROUP];
#pragma unroll
    for (int e = 0; e < NV_GROUP; ++e) acc[e] = 0.0;
    frame_terms<Bac, NK, 12>(g, g.frm_off[f], g.frm_off[f + 1], tid, acc);
    block_fold_f64<NV_GROUP>(acc, wred, tot);
    if (tid < NV_GROUP) g.fpart[(size_t)f * NV_GROUP + tid] = tot[tid];
}

// A group's fold over its frames' partials (rows of NV values), the blocked order over the group's list, by one workgroup: thread
// t owns value t % NV of the blocks t / NV, t / NV + blockDim.x / NV, ... (a block's rows added to 0.0 in ascending order) and
// leaves each block's sum in blk; then thread e < NV adds the block sums to 0.0 in ascending order.  Every thread may read tot
// [NV] (LDS) after the call.  blk: the group's part of the workspace's fold buffer, (end - beg) / BLK + 1 rows at most.
template <int NV>
__device__ void group_fold(const double* __restrict__ part, const int* __restrict__ frames, int beg, int end, double* blk, double* tot) {
    const int tid = threadIdx.x, e = tid % NV, per = blockDim.x / NV, nb = cdiv_d(end - beg, BLK);
    if (tid / NV < per)
        for (int b = tid / NV; b < nb; b += per) {
            const int a = beg + b * BLK, z = a + BLK < end ? a + BLK : end;
            double s = 0.0;
            for (int i = a; i < z; ++i) s += part[(size_t)frames[i] * NV + e];
            blk[(size_t)b * NV + e] = s;
        }
    __syncthreads();
    if (tid < NV) {
        double total = 0.0;
        for (int b = 0; b < nb; ++b) total += blk[(size_t)b * NV + tid];
        tot[tid] = total;
    }
    __syncthreads();
}

// where group q's block sums start in the fold buffer: the groups before it fill grp_off[q] / BLK + q rows at most
__device__ __forceinline__ double* fold_rows(const Bac& g, int q, int nv) { return g.gfold + ((size_t)(g.grp_off[q] / BLK) + q) * nv; }

// A x = b for a symmetric 8 x 8 A (36 upper-triangle values) by Cholesky, chol_solve6's steps; false when a pivot is not positive
// or x is not finite
__device__ bool chol_solve8(const double* __restrict__ Au, const double* b, double* x) {
    double L[NK][NK];
#pragma unroll
    for (int i = 0; i < NK; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < k; ++j) s += L[i][j] * L[k][j];
            s = Au[k * NK - k * (k - 1) / 2 + (i - k)] - s;      // A[k][i], k <= i
            if (i == k) {
                if (!(s > 0.0)) return false;
                L[i][i] = sqrt(s);
            } else {
                L[i][k] = s / L[k][k];
            }
        }
    double y[NK];
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < i; ++j) s += L[i][j] * y[j];
        y[i] = (b[i] - s) / L[i][i];
    }
    bool okx = true;
#pragma unroll
    for (int i = NK - 1; i >= 0; --i) {
        double s = 0.0;
#pragma unroll
        for (int j = i + 1; j < NK; ++j) s += L[j][i] * x[j];
        x[i] = (y[i] - s) / L[i][i];
        okx = okx && fin(x[i]);
    }
    return okx;
}

__device__ __forceinline__ void precond8(const double* __restrict__ S, const double* r, double* z) {
    if (!chol_solve8(S, r, z)) {
#pragma unroll
        for (int a = 0; a < NK; ++a) z[a] = r[a];
    }
}

// one workgroup of 1024 per group: the fold of its frames' sums, then the group's block (damped; a frozen parameter's diagonal
// 1), diag U_k and b_k = W_k V^-1 g_p - g_k
__global__ __launch_bounds__(1024) void bac_groups_kernel(Bac g) {
    __shared__ double tot[NV_GROUP];
    if (g.si[SI_DONE]) return;
    const int q = blockIdx.x, tid = threadIdx.x;
    group_fold<NV_GROUP>(g.fpart, g.grp_frame, g.grp_off[q], g.grp_off[q + 1], fold_rows(g, q, NV_GROUP), tot);
    if (tid != 0) return;
    const double lam = g.sd[SD_LAM];
    const int mask = g.gmask[q];
    double* S = g.Sg + (size_t)q * 36;
    int e = 0;
    for (int a = 0; a < NK; ++a)
        for (int c = a; c < NK; ++c) {
            double v = tot[e];
            if (a == c) v = ((mask >> a) & 1) ? 1.0 : v + lam * tot[36 + a];
            S[e++] = v;
        }
    for (int a = 0; a < NK; ++a) {
        g.dUg[(size_t)q * NK + a] = tot[36 + a];
        g.bg[(size_t)q * NK + a] = tot[52 + a] - tot[44 + a];
    }
}

// ---------------------------------------------------------------- conjugate gradients on S d_c = b
// a dot product's total: over the frames, then (with groups) over the groups, the two added frames first; which: 0 / 1, the half
// of fdot / gdot
template <class G>
__device__ double dot_total(const G& g, int which, double* sh) {
    double s = blocked_sum(g.fdot + (size_t)which * g.F, g.F, g.part + which * cdiv_d(g.F, BLK), sh);
    if constexpr (G::CAM) s = s + blocked_sum(g.gdot + (size_t)which * g.G, g.G, g.gpart + which * cdiv_d(g.G, BLK), sh);
    return s;
}

// one thread per group: the group's rows of the start of a solve
__global__ __launch_bounds__(256) void bac_cg_init_kernel(Bac g) {
    if (g.si[SI_DONE]) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.G) return;
    double r[NK], z[NK];
#pragma unroll
    for (int a = 0; a < NK; ++a) r[a] = g.bg[(size_t)q * NK + a];
    precond8(g.Sg + (size_t)q * 36, r, z);
    double rz = 0.0, rr = 0.0;
#pragma unroll
    for (int a = 0; a < NK; ++a) {
        const size_t i = (size_t)q * NK + a;
        g.gx[i] = 0.0; g.gr[i] = r[a]; g.gz[i] = z[a]; g.gpv[i] = z[a];
        rz += r[a] * z[a]; rr += r[a] * r[a];
    }
    g.gdot[q] = rz; g.gdot[g.G + q] = rr;
}

__global__ __launch_bounds__(256) void bac_cg_update_kernel(Bac g) {
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.G) return;
    const double alpha = g.sd[SD_ALPHA];
    double r[NK], z[NK];
#pragma unroll
    for (int a = 0; a < NK; ++a) {
        const size_t i = (size_t)q * NK + a;
        g.gx[i] = g.gx[i] + alpha * g.gpv[i];
        r[a] = g.gr[i] - alpha * g.gq[i];
        g.gr[i] = r[a];
    }
    precond8(g.Sg + (size_t)q * 36, r, z);
    double rz = 0.0, rr = 0.0;
#pragma unroll
    for (int a = 0; a < NK; ++a) { g.gz[(size_t)q * NK + a] = z[a]; rz += r[a] * z[a]; rr += r[a] * r[a]; }
    g.gdot[q] = rz; g.gdot[g.G + q] = rr;
}

__global__ __launch_bounds__(256) void bac_cg_dir_kernel(Bac g) {
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < g.G * NK) g.gpv[i] = g.gz[i] + g.sd[SD_BETA] * g.gpv[i];
}

// one workgroup of 256 per group, the third pass of a matvec: q_g = the fold of its frames' sum J_k^T t, plus lam diag(U_k) v_g;
// a frozen parameter's row the identity; v_g . q_g
__global__ __launch_bounds__(256) void bac_mv_groups_kernel(Bac g) {
    __shared__ double tot[NK];
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const int q = blockIdx.x, tid = threadIdx.x;
    group_fold<NK>(g.mvpart, g.grp_frame, g.grp_off[q], g.grp_off[q + 1], fold_rows(g, q, NK), tot);
    if (tid != 0) return;
    const double lam = g.sd[SD_LAM];
    const int mask = g.gmask[q];
    double pq = 0.0;
    for (int a = 0; a < NK; ++a) {
        const double va = g.gpv[(size_t)q * NK + a];
        const double qa = ((mask >> a) & 1) ? va : tot[a] + lam * g.dUg[(size_t)q * NK + a] * va;
        g.gq[(size_t)q * NK + a] = qa;
        pq += va * qa;
    }
    g.gdot[q] = pq;
}

__global__ __launch_bounds__(256) void ba_cg_init_kernel(Ba g) {
    if (g.si[SI_DONE]) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f == 0) { g.si[SI_CG_ITER] = 0; g.si[SI_CG_DONE] = 0; }
    if (f >= g.F) return;
    double r[6], z[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) r[a] = g.b[(size_t)f * 6 + a];
    precond(g.Sblk + (size_t)f * 21, r, z);
    double rz = 0.0, rr = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        g.x[(size_t)f * 6 + a] = 0.0; g.r[(size_t)f * 6 + a] = r[a]; g.z[(size_t)f * 6 + a] = z[a]; g.p[(size_t)f * 6 + a] = z[a];
        rz += r[a] * z[a]; rr += r[a] * r[a];
    }
    g.fdot[f] = rz; g.fdot[g.F + f] = rr;
}

template <class G>
__global__ __launch_bounds__(256) void ba_cg_start_kernel(G g) {
    __shared__ double sh[1];
    if (g.si[SI_DONE]) return;
    const double rz = dot_total(g, 0, sh), bb = dot_total(g, 1, sh);
    if (threadIdx.x == 0) {
        g.sd[SD_RZ] = rz; g.sd[SD_BB] = bb; g.sd[SD_RR] = bb;
        if (!(bb > 0.0)) g.si[SI_CG_DONE] = 1;      // b = 0 (or not a number): d_c = 0
    }
}

// one wave per point.  mode 0: y_p = V^-1 sum J_p^T J_c v_c (the first pass of a matvec); mode 1: the back-substitution
// d_p = -V^-1 (g_p + sum J_p^T J_c d_c) and the candidate point
// With groups the sum under J_p^T is J_c v_f + J_k v_g(f), the group's part added behind the pose's (vec: cg_p or cg_x, and the
// groups' vector of the same kind).
template <class G>
__global__ __launch_bounds__(64) void ba_mv_points_kernel(G g, const double* __restrict__ vec, int mode) {
    constexpr int JW = G::JW, OP = G::JW - 8;
    if (g.si[SI_DONE] || (mode == 0 && g.si[SI_CG_DONE])) return;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int beg = g.pt_off[p], end = g.pt_off[p + 1];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = beg + lane; k < end; k += 64) {
        const int o = g.pt_obs[k];
        const double* j = g.J + (size_t)o * JW;
        const int f = g.obs_frame[o];
        const double* v = vec + (size_t)f * 6;
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { t0 += j[a] * v[a]; t1 += j[6 + a] * v[a]; }
        if constexpr (G::CAM) {
            const double* w = (mode == 0 ? g.gpv : g.gx) + (size_t)g.frm_grp[f] * NK;
#pragma unroll
            for (int a = 0; a < NK; ++a) { t0 += j[12 + a] * w[a]; t1 += j[12 + NK + a] * w[a]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += j[OP + c] * t0 + j[OP + 3 + c] * t1;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = wave_sum_f64(acc[c]);
    if (lane != 0) return;
    const double* V = g.Vinv + (size_t)p * 6;
    double y[3];
    if (mode == 0) {
        vinv_mul(V, acc, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) g.yp[(size_t)p * 3 + c] = y[c];
    } else {
        const double s[3] = {g.gp[(size_t)p * 3] + acc[0], g.gp[(size_t)p * 3 + 1] + acc[1], g.gp[(size_t)p * 3 + 2] + acc[2]};
        vinv_mul(V, s, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) g.Xc[(size_t)p * 3 + c] = g.X[(size_t)p * 3 + c] - y[c];
    }
}

// one workgroup per frame: q_f = (U + lam diag U) p_f - sum J_c^T J_p y_p, a frozen parameter's row the identity; p_f . q_f
// With groups t also holds J_k v_g, and the frame's sum J_k^T t (8 values) goes to mvpart for bac_mv_groups_kernel.
template <class G>
__global__ __launch_bounds__(256) void ba_mv_frames_kernel(G g) {
    constexpr int JW = G::JW, OP = G::JW - 8, NA = G::CAM ? 6 + NK : 6;
    __shared__ double wred[4][NA], tot[NA];
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int beg = g.frm_off[f], end = g.frm_off[f + 1];
    double v[6], acc[NA];
    [[maybe_unused]] double w[NK];
#pragma unroll
    for (int a = 0; a < 6; ++a) v[a] = g.p[(size_t)f * 6 + a];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    if constexpr (G::CAM) {
#pragma unroll
        for (int a = 0; a < NK; ++a) w[a] = g.gpv[(size_t)g.frm_grp[f] * NK + a];
    }
    for (int o = beg + tid; o < end; o += 256) {
        const double* j = g.J + (size_t)o * JW;
        const double* y = g.yp + (size_t)g.obs_point[o] * 3;
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { t0 += j[a] * v[a]; t1 += j[6 + a] * v[a]; }
        if constexpr (G::CAM) {
#pragma unroll
            for (int a = 0; a < NK; ++a) { t0 += j[12 + a] * w[a]; t1 += j[12 + NK + a] * w[a]; }
        }
        t0 -= j[OP] * y[0] + j[OP + 1] * y[1] + j[OP + 2] * y[2];
        t1 -= j[OP + 3] * y[0] + j[OP + 4] * y[1] + j[OP + 5] * y[2];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] += j[a] * t0 + j[6 + a] * t1;
        if constexpr (G::CAM) {
#pragma unroll
            for (int a = 0; a < NK; ++a) acc[6 + a] += j[12 + a] * t0 + j[12 + NK + a] * t1;
        }
    }
    block_fold_f64<NA>(acc, wred, tot);
    if constexpr (G::CAM) {
        if (tid < NK) g.mvpart[(size_t)f * NK + tid] = tot[6 + tid];
    }
    if (tid != 0) return;
    const double lam = g.sd[SD_LAM];
    const int mask = g.fmask[f];
    double pq = 0.0;
    for (int a = 0; a < 6; ++a) {
        const double qa = ((mask >> a) & 1) ? v[a] : tot[a] + lam * g.dU[(size_t)f * 6 + a] * v[a];
        g.q[(size_t)f * 6 + a] = qa;
        pq += v[a] * qa;
    }
    g.fdot[f] = pq;
}

template <class G>
__global__ __launch_bounds__(256) void ba_cg_alpha_kernel(G g) {
    __shared__ double sh[1];
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const double pap = dot_total(g, 0, sh);
    if (threadIdx.x == 0) {
        const double alpha = g.sd[SD_RZ] / pap;
        g.sd[SD_PAP] = pap;
        if (!(pap > 0.0) || !fin(alpha)) { g.si[SI_CG_DONE] = 1; g.si[SI_CG_FAIL] += 1; g.sd[SD_ALPHA] = 0.0; }      // the step so far stands
        else g.sd[SD_ALPHA] = alpha;
    }
}

__global__ __launch_bounds__(256) void ba_cg_update_kernel(Ba g) {
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= g.F) return;
    const double alpha = g.sd[SD_ALPHA];
    double r[6], z[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const size_t i = (size_t)f * 6 + a;
        g.x[i] = g.x[i] + alpha * g.p[i];
        r[a] = g.r[i] - alpha * g.q[i];
        g.r[i] = r[a];
    }
    precond(g.Sblk + (size_t)f * 21, r, z);
    double rz = 0.0, rr = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) { g.z[(size_t)f * 6 + a] = z[a]; rz += r[a] * z[a]; rr += r[a] * r[a]; }
    g.fdot[f] = rz; g.fdot[g.F + f] = rr;
}

template <class G>
__global__ __launch_bounds__(256) void ba_cg_beta_kernel(G g) {
    __shared__ double sh[1];
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const double rz = dot_total(g, 0, sh), rr = dot_total(g, 1, sh);
    if (threadIdx.x == 0) {
        const double beta = rz / g.sd[SD_RZ];
        g.sd[SD_BETA] = beta; g.sd[SD_RZ] = rz; g.sd[SD_RR] = rr;
        g.si[SI_CG_ITER] += 1;
        if (sqrt(rr) <= g.sd[SD_CGTOL] * sqrt(g.sd[SD_BB]) || !fin(beta)) g.si[SI_CG_DONE] = 1;
    }
}

__global__ __launch_bounds__(256) void ba_cg_dir_kernel(Ba g) {
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < g.F * 6) g.p[i] = g.z[i] + g.sd[SD_BETA] * g.p[i];
}

// ---------------------------------------------------------------- candidate, cost, decision
__global__ __launch_bounds__(256) void ba_pose_cand_kernel(Ba g) {
    if (g.si[SI_DONE]) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= g.F) return;
    const double* T = g.T + (size_t)f * FC;
    double* O = g.Tc + (size_t)f * FC;
    double d[6];
    bool still = true;
#pragma unroll
    for (int a = 0; a < 6; ++a) { d[a] = g.x[(size_t)f * 6 + a]; still = still && d[a] == 0.0; }
    if (still) {      // bit for bit: a frame that does not move keeps its row
        for (int e = 0; e < FC; ++e) O[e] = T[e];
        return;
    }
    Pose q, c;
    for (int e = 0; e < 9; ++e) q.R[e] = T[e];
    for (int e = 0; e < 3; ++e) q.t[e] = T[9 + e];
    pose_update(q, d, c);
    for (int e = 0; e < 9; ++e) O[e] = c.R[e];
    for (int e = 0; e < 3; ++e) O[9 + e] = c.t[e];
    O[12] = -(c.R[0] * c.t[0] + c.R[3] * c.t[1] + c.R[6] * c.t[2]);
    O[13] = -(c.R[1] * c.t[0] + c.R[4] * c.t[1] + c.R[7] * c.t[2]);
    O[14] = -(c.R[2] * c.t[0] + c.R[5] * c.t[1] + c.R[8] * c.t[2]);
    O[15] = T[15];
}

// one workgroup per frame: the frame's share of the cost at the accepted state (cand 0) or at the candidate (cand 1)
__global__ __launch_bounds__(256) void ba_cost_kernel(Ba g, int cand) {
    __shared__ double wred[4][1], tot[1];
    if (g.si[SI_DONE]) return;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int beg = g.frm_off[f], end = g.frm_off[f + 1];
    const double* table = cand ? g.Tc : g.T;
    const double* xyz = cand ? g.Xc : g.X;
    const Obs og = obs_view(g, table);
    const double loss2 = g.sd[SD_LOSS2];
    double acc[1] = {0.0};
    for (int o = beg + tid; o < end; o += 256) {
        const int p = g.obs_point[o];
        const V3 X = {xyz[(size_t)p * 3], xyz[(size_t)p * 3 + 1], xyz[(size_t)p * 3 + 2]};
        double z, r0, r1;
        obs_residual(og, g.obs_row[o], f, X, z, r0, r1, false, nullptr);
        const double s = (r0 * r0 + r1 * r1) / loss2;
        if (z > 1e-12 && fin(s)) acc[0] += log1p(s);
    }
    block_fold_f64<1>(acc, wred, tot);
    if (tid == 0) g.fcost[f] = tot[0];
}

// the one decision of an iteration: pose.hip's rule (accept when the cost falls, lam x 0.1 / x 10, a NaN cost rejects)
__global__ __launch_bounds__(256) void ba_decide_kernel(Ba g, int initial) {
    __shared__ double sh[1];
    if (g.si[SI_DONE]) return;
    const double c = blocked_sum(g.fcost, g.F, g.part, sh);
    if (threadIdx.x != 0) return;
    if (initial) {
        g.sd[SD_COST] = c; g.sd[SD_COST0] = c; g.sd[SD_CAND] = c;
        if (g.max_iters == 0) { g.si[SI_DONE] = 1; g.si[SI_REASON] = PRAM_BA_REASON_MAX_ITERS; }
        return;
    }
    const int it = g.si[SI_LM_ITER];
    const double cost = g.sd[SD_COST];
    const bool accept = c < cost;
    g.sd[SD_CAND] = c;
    if (it < g.max_iters) { g.si[PRAM_BA_STATE_I32 + it] = g.si[SI_CG_ITER]; g.si[PRAM_BA_STATE_I32 + g.max_iters + it] = accept; }
    g.si[SI_PENDING] = accept; g.si[SI_RELIN] = accept;
    if (accept) {
        g.sd[SD_COST] = c;
        g.sd[SD_LAM] = fmax(g.sd[SD_LAM] * 0.1, 1e-15);
        g.si[SI_ACCEPTED] += 1;
        if ((cost - c) / cost < g.sd[SD_FTOL]) { g.si[SI_DONE] = 1; g.si[SI_REASON] = PRAM_BA_REASON_FTOL; }
    } else {
        g.sd[SD_LAM] = g.sd[SD_LAM] * 10.0;
    }
    g.si[SI_LM_ITER] = it + 1;
    if (it + 1 >= g.max_iters && !g.si[SI_DONE]) { g.si[SI_DONE] = 1; g.si[SI_REASON] = PRAM_BA_REASON_MAX_ITERS; }
}

// an accepted candidate becomes the state (the copy is the same whenever it is repeated, so it does not look at `done`)
__global__ __launch_bounds__(256) void ba_apply_kernel(Ba g) {
    if (!g.si[SI_PENDING] || g.si[SI_BAD]) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)g.F * FC) g.T[i] = g.Tc[i];
    if (i < (long long)g.P * 3) g.X[i] = g.Xc[i];
    if (i < g.F) {
        bool mv = false;
        for (int a = 0; a < 6; ++a) mv = mv || g.x[(size_t)i * 6 + a] != 0.0;
        if (mv) g.moved[i] = 1;
    }
}

// ---------------------------------------------------------------- camera groups: tables, parameters, candidate
// Every index a later kernel reads through the group tables, once, as ba_check_kernel does for the observation tables: the CSR's
// offsets, every grp_frame in range and ascending within its group, frm_grp the CSR's inverse (so every frame is in exactly one
// group), one model per group.  One thread per frame (CSR entry) and per group.
__global__ __launch_bounds__(256) void bac_check_kernel(Bac g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && (g.grp_off[0] != 0 || g.grp_off[g.G] != g.F)) ba_bad(g);
    if (i < g.G) {
        const int a = g.grp_off[i], b = g.grp_off[i + 1];
        if (a < 0 || b < a || b > g.F) ba_bad(g);
    }
    if (i < g.F) {
        const int q = g.frm_grp[i], f = g.grp_frame[i];
        bool ok = q >= 0 && q < g.G && f >= 0 && f < g.F;
        if (ok) {
            // entry i of the CSR belongs to the group h with grp_off[h] <= i < grp_off[h + 1]
            const int h = first_true(0, g.G - 1, [&](int k) { return g.grp_off[k + 1] > i; });
            const int a = g.grp_off[h], b = g.grp_off[h + 1];
            ok = a >= 0 && a <= i && i < b && b <= g.F && g.frm_grp[f] == h;
            if (ok && i > a) { const int e = g.grp_frame[i - 1]; ok = e >= 0 && e < f; }
            if (ok) { const int f0 = g.grp_frame[a]; ok = f0 >= 0 && f0 < g.F && g.cam_model[f0] == g.cam_model[f]; }
        }
        if (!ok) ba_bad(g);
    }
}

// one thread per group: its model, its mask (the caller's bits, the parameters the model does not have, and everything when the
// group has no observations), its parameters
__global__ __launch_bounds__(256) void bac_setup_kernel(Bac g) {
    if (g.si[SI_BAD]) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.G) return;
    const int a = g.grp_off[q], b = g.grp_off[q + 1];
    const int model = b > a ? g.cam_model[g.grp_frame[a]] : PRAM_CAM_SIMPLE_PINHOLE;
    int n = 0;
    for (int i = a; i < b && n == 0; ++i) { const int f = g.grp_frame[i]; n = g.frm_off[f + 1] - g.frm_off[f]; }
    const int absent = 255 & ~((1 << cam_n_params(model)) - 1);
    g.gmodel[q] = model;
    g.gmask[q] = n > 0 ? ((g.grp_mask_in[q] & 255) | absent) : 255;
    g.gbad[q] = 0;
    for (int e = 0; e < NK; ++e) { const double v = g.grp_params_in[(size_t)q * NK + e]; g.k[(size_t)q * NK + e] = v; g.kc[(size_t)q * NK + e] = v; }
}

// the per-frame parameters obs_residual reads, from the groups' accepted (cand 0) or candidate (cand 1) parameters
__global__ __launch_bounds__(256) void bac_expand_kernel(Bac g, int cand) {
    if (g.si[SI_BAD] || (cand && g.si[SI_DONE])) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.F * NK) return;
    const double* src = cand ? g.kc : g.k;
    (cand ? g.cpc : g.cp)[i] = src[(size_t)g.frm_grp[i / NK] * NK + i % NK];
}

// one thread per group: k + d_k; a group whose step is 0 keeps its parameters bit for bit; a focal length that is not finite or
// not above 0 marks the candidate
__global__ __launch_bounds__(256) void bac_cand_kernel(Bac g) {
    if (g.si[SI_DONE]) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.G) return;
    const int nf = cam_n_focal(g.gmodel[q]);
    bool bad = false;
    for (int a = 0; a < NK; ++a) {
        const double d = g.gx[(size_t)q * NK + a], v = g.k[(size_t)q * NK + a];
        const double c = d == 0.0 ? v : v + d;
        g.kc[(size_t)q * NK + a] = c;
        if (a < nf) bad = bad || !fin(c) || !(c > 0.0);
    }
    g.gbad[q] = bad;
}

// behind ba_cost_kernel at the candidate: a frame of a marked group makes the candidate's cost NaN, which the decision rejects
__global__ __launch_bounds__(256) void bac_poison_kernel(Bac g) {
    if (g.si[SI_DONE]) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < g.F && g.gbad[g.frm_grp[f]]) g.fcost[f] = nan("");
}

// the groups' share of ba_apply_kernel
__global__ __launch_bounds__(256) void bac_apply_kernel(Bac g) {
    if (!g.si[SI_PENDING] || g.si[SI_BAD]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < g.F * NK) g.cp[i] = g.cpc[i];
    if (i < g.G * NK) g.k[i] = g.kc[i];
}

__global__ __launch_bounds__(256) void bac_params_out_kernel(Bac g, double* __restrict__ out) {
    if (g.si[SI_BAD]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < g.G * NK) out[i] = g.k[i];
}

// ---------------------------------------------------------------- the filter after the last iteration
__global__ __launch_bounds__(256) void ba_filter_obs_kernel(Ba g, double thr2, unsigned char* __restrict__ keep, double* __restrict__ err,
                                                            int* __restrict__ counts) {
    if (g.si[SI_BAD]) return;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= g.n_obs) return;
    const int p = g.obs_point[o];
    const V3 X = {g.X[(size_t)p * 3], g.X[(size_t)p * 3 + 1], g.X[(size_t)p * 3 + 2]};
    double z, r0, r1;
    obs_residual(obs_view(g, g.T), g.obs_row[o], g.obs_frame[o], X, z, r0, r1, false, nullptr);
    const double e2 = r0 * r0 + r1 * r1;
    const bool in = z > 0.0 && e2 <= thr2;      // obs_inlier's test
    keep[o] = in;
    err[o] = sqrt(e2);
    if (!(z > 1e-12) || !fin(e2 / g.sd[SD_LOSS2])) atomicAdd(counts, 1);          // the observations of weight 0 at the final state
    if (!in) atomicAdd(counts + 1, 1);
}

// one wave per point: the kept observations, their mean error, and the largest angle between the rays of two of them (the pairs
// strided over the lanes by their first member)
__global__ __launch_bounds__(64) void ba_filter_points_kernel(Ba g, const unsigned char* __restrict__ keep, const double* __restrict__ err,
                                                              double min_angle, int* __restrict__ pt_keep, double* __restrict__ pt_err,
                                                              double* __restrict__ pt_angle, int* __restrict__ pt_cnt) {
    if (g.si[SI_BAD]) return;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int beg = g.pt_off[p], end = g.pt_off[p + 1];
    const V3 X = {g.X[(size_t)p * 3], g.X[(size_t)p * 3 + 1], g.X[(size_t)p * 3 + 2]};
    const Obs og = obs_view(g, g.T);
    int cnt = 0;
    double esum = 0.0, best = -1.0;
    for (int k = beg + lane; k < end; k += 64) {
        const int o = g.pt_obs[k];
        if (!keep[o]) continue;
        cnt += 1;
        esum += err[o];
        const V3 vi = sub(X, obs_centre(og, g.obs_frame[o]));
        for (int m = k + 1; m < end; ++m) {
            const int o2 = g.pt_obs[m];
            if (!keep[o2]) continue;
            const double a = angle(vi, sub(X, obs_centre(og, g.obs_frame[o2])));
            if (a > best) best = a;
        }
    }
    cnt = wave_sum_i32(cnt);
    esum = wave_sum_f64(esum);
    best = wave_max_f64(best);
    if (lane != 0) return;
    pt_keep[p] = cnt >= 2 && best >= min_angle;
    pt_err[p] = cnt > 0 ? esum / (double)cnt : 0.0;
    pt_angle[p] = best;
    pt_cnt[p] = cnt;
}

// a frame that moved gets its pose from the table; one that never did keeps the caller's numbers bit for bit
__global__ __launch_bounds__(256) void ba_poses_out_kernel(Ba g, const double* __restrict__ qvec_in, const double* __restrict__ tvec_in,
                                                           double* __restrict__ qvec, double* __restrict__ tvec) {
    if (g.si[SI_BAD]) return;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= g.F) return;
    if (!g.moved[f]) {
        for (int a = 0; a < 4; ++a) qvec[(size_t)f * 4 + a] = qvec_in[(size_t)f * 4 + a];
        for (int a = 0; a < 3; ++a) tvec[(size_t)f * 3 + a] = tvec_in[(size_t)f * 3 + a];
        return;
    }
    double qv[4];
    rot_to_qvec(g.T + (size_t)f * FC, qv);
    for (int a = 0; a < 4; ++a) qvec[(size_t)f * 4 + a] = qv[a];
    for (int a = 0; a < 3; ++a) tvec[(size_t)f * 3 + a] = g.T[(size_t)f * FC + 9 + a];
}

// ---------------------------------------------------------------- host side
size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

constexpr int MAX_OBS = 1 << 26, MAX_ITERS = 4096;      // 20 doubles an observation: the Jacobians of 2^26 take 10 GB

bool sizes_ok(int F, int P, int n_obs, int max_iters) {
    return F >= 1 && P >= 1 && n_obs >= 1 && F <= (1 << 24) && P <= (1 << 28) && n_obs <= MAX_OBS && max_iters >= 0 && max_iters <= MAX_ITERS;
}

// offsets [PRAM_BA_ARRAYS + 1] of the workspace's arrays, the last one the total; jw: the doubles of an observation's row
void layout(int F, int P, int n_obs, int max_iters, size_t* off, int jw = JW) {
    const size_t d = sizeof(double), i = sizeof(int), nb = (size_t)cdiv(F, BLK);
    const size_t bytes[A_COUNT] = {(size_t)F * FC * d, (size_t)F * FC * d, (size_t)P * 3 * d, (size_t)P * 3 * d, (size_t)n_obs * jw * d, (size_t)P * 6 * d,
                                   (size_t)P * 3 * d, (size_t)P * 3 * d, (size_t)F * 21 * d, (size_t)F * 6 * d, (size_t)F * 6 * d, (size_t)F * 6 * d,
                                   (size_t)F * 6 * d, (size_t)F * 6 * d, (size_t)F * 6 * d, (size_t)F * 6 * d, (size_t)F * 2 * d, (size_t)F * d, 2 * nb * d,
                                   (size_t)PRAM_BA_STATE_F64 * d, (size_t)(PRAM_BA_STATE_I32 + 2 * max_iters) * i, (size_t)P * i, (size_t)F * i,
                                   (size_t)F * i, (size_t)n_obs};
    off[0] = 0;
    for (int a = 0; a < A_COUNT; ++a) off[a + 1] = off[a] + al(bytes[a]);
}

// offsets [PRAM_BAC_ARRAYS + 1]: the arrays above with rows of PRAM_BAC_OBS_DOUBLES, then the groups'
void layout_cam(int F, int P, int n_obs, int G, int max_iters, size_t* off) {
    layout(F, P, n_obs, max_iters, off, PRAM_BAC_OBS_DOUBLES);
    const size_t d = sizeof(double), i = sizeof(int), nb = (size_t)cdiv(G, BLK), g = (size_t)G;
    const size_t bytes[C_COUNT - A_COUNT] = {(size_t)F * NK * d, (size_t)F * NK * d, g * NK * d, g * NK * d, g * 36 * d, g * NK * d, g * NK * d, g * NK * d,
                                             g * NK * d, g * NK * d, g * NK * d, g * NK * d, g * 2 * d, 2 * nb * d, (size_t)F * NV_GROUP * d,
                                             (size_t)F * NK * d, g * i, g * i, g * i, ((size_t)(F / BLK) + g + 1) * NV_GROUP * d};
    for (int a = A_COUNT; a < C_COUNT; ++a) off[a + 1] = off[a] + al(bytes[a - A_COUNT]);
}

bool sizes_cam_ok(int F, int P, int n_obs, int G, int max_iters) { return sizes_ok(F, P, n_obs, max_iters) && G >= 1 && G <= F; }

int load_ctx(const void* ctx, Ba* g, const char* what) {
    PRAM_REQUIRE(ctx, "%s: null context", what);
    memcpy(g, ctx, sizeof(Ba));
    PRAM_REQUIRE(g->magic == MAGIC, "%s: the context is not one pram_ba_begin filled", what);
    return PRAM_OK;
}

int load_ctx_cam(const void* ctx, Bac* g, const char* what) {
    PRAM_REQUIRE(ctx, "%s: null context", what);
    memcpy(static_cast<void*>(g), ctx, sizeof(Bac));
    PRAM_REQUIRE(g->magic == MAGIC_CAM, "%s: the context is not one pram_bac_begin filled", what);
    return PRAM_OK;
}

Ba make_base(const float* keypoints, const int* cam_model, const double* cam_params, const int* obs_row, const int* obs_frame, const int* obs_point,
             const int* frm_off, const int* pt_off, const int* pt_obs, const int* frozen, int F, int P, int n_obs, int n_rows, int max_iters, char* w,
             const size_t* off, unsigned long long magic) {
    const auto D = [&](int a) { return reinterpret_cast<double*>(w + off[a]); };
    const auto I = [&](int a) { return reinterpret_cast<int*>(w + off[a]); };
    Ba g = {keypoints, cam_model, cam_params, obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen, F, P, n_obs, n_rows,
            max_iters, D(A_T), D(A_TC), D(A_X), D(A_XC), D(A_J), D(A_VINV), D(A_GP), D(A_YP), D(A_SBLK), D(A_DU), D(A_B), D(A_CGX), D(A_CGR),
            D(A_CGZ), D(A_CGP), D(A_CGQ), D(A_FDOT), D(A_FCOST), D(A_PART), D(A_SD), I(A_SI), I(A_PFLAG), I(A_MOVED), I(A_FMASK),
            reinterpret_cast<unsigned char*>(w + off[A_OOK]), magic};
    return g;
}

// the state, the tables' check, the copies of the poses and points, the initial cost: with groups also their check, their
// parameters and the per-frame parameters the cost reads
template <class G>
void enqueue_begin(const G& g, const double* table, const double* xyz, double loss_scale, double lam0, double cg_tol, double ftol, hipStream_t st) {
    const Ba& b = g;
    const int F = g.F, P = g.P;
    const int most = g.n_obs > F ? (g.n_obs > P ? g.n_obs : P) : (F > P ? F : P);
    hipLaunchKernelGGL(ba_init_kernel, dim3(1), dim3(1), 0, st, b, loss_scale, lam0, cg_tol, ftol);
    hipLaunchKernelGGL(ba_check_kernel, dim3(cdiv(most, 256)), dim3(256), 0, st, b);
    if constexpr (G::CAM) {
        hipLaunchKernelGGL(bac_check_kernel, dim3(cdiv(F, 256)), dim3(256), 0, st, g);
        hipLaunchKernelGGL(bac_setup_kernel, dim3(cdiv(g.G, 256)), dim3(256), 0, st, g);
        hipLaunchKernelGGL(bac_expand_kernel, dim3(cdiv(F * NK, 256)), dim3(256), 0, st, g, 0);
        hipLaunchKernelGGL(bac_expand_kernel, dim3(cdiv(F * NK, 256)), dim3(256), 0, st, g, 1);
    }
    const long long nt = (long long)F * FC, nx = (long long)P * 3;
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, table, g.T, nt);
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, table, g.Tc, nt);
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, xyz, g.X, nx);
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, xyz, g.Xc, nx);
    hipLaunchKernelGGL(ba_cost_kernel, dim3(F), dim3(256), 0, st, b, 0);
    hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(256), 0, st, b, 1);
}

template <class G>
void enqueue_iterations(const G& g, int n_iters, int cg_iters, int stages, hipStream_t st) {
    const Ba& b = g;
    const int F = g.F, P = g.P;
    const dim3 per_frame(cdiv(F, 256)), per_unknown(cdiv(F * 6, 256));
    for (int it = 0; it < n_iters; ++it) {
        if (stages & PRAM_BA_STAGE_LINEARISE) hipLaunchKernelGGL(ba_linearise_kernel<G>, dim3(cdiv(g.n_obs, 256)), dim3(256), 0, st, g);
        if (stages & PRAM_BA_STAGE_BLOCKS) {
            hipLaunchKernelGGL(ba_points_kernel<G>, dim3(P), dim3(64), 0, st, g);
            hipLaunchKernelGGL(ba_frames_kernel<G>, dim3(F), dim3(256), 0, st, g);
            if constexpr (G::CAM) {
                hipLaunchKernelGGL(bac_frames_kernel, dim3(F), dim3(256), 0, st, g);
                hipLaunchKernelGGL(bac_groups_kernel, dim3(g.G), dim3(1024), 0, st, g);
            }
        }
        if (stages & PRAM_BA_STAGE_CG_INIT) {
            hipLaunchKernelGGL(ba_cg_init_kernel, per_frame, dim3(256), 0, st, b);
            if constexpr (G::CAM) hipLaunchKernelGGL(bac_cg_init_kernel, dim3(cdiv(g.G, 256)), dim3(256), 0, st, g);
            hipLaunchKernelGGL(ba_cg_start_kernel<G>, dim3(1), dim3(256), 0, st, g);
        }
        if (stages & PRAM_BA_STAGE_CG)
            for (int k = 0; k < cg_iters; ++k) {
                hipLaunchKernelGGL(ba_mv_points_kernel<G>, dim3(P), dim3(64), 0, st, g, (const double*)g.p, 0);
                hipLaunchKernelGGL(ba_mv_frames_kernel<G>, dim3(F), dim3(256), 0, st, g);
                if constexpr (G::CAM) hipLaunchKernelGGL(bac_mv_groups_kernel, dim3(g.G), dim3(256), 0, st, g);
                hipLaunchKernelGGL(ba_cg_alpha_kernel<G>, dim3(1), dim3(256), 0, st, g);
                hipLaunchKernelGGL(ba_cg_update_kernel, per_frame, dim3(256), 0, st, b);
                if constexpr (G::CAM) hipLaunchKernelGGL(bac_cg_update_kernel, dim3(cdiv(g.G, 256)), dim3(256), 0, st, g);
                hipLaunchKernelGGL(ba_cg_beta_kernel<G>, dim3(1), dim3(256), 0, st, g);
                hipLaunchKernelGGL(ba_cg_dir_kernel, per_unknown, dim3(256), 0, st, b);
                if constexpr (G::CAM) hipLaunchKernelGGL(bac_cg_dir_kernel, dim3(cdiv(g.G * NK, 256)), dim3(256), 0, st, g);
            }
        if (stages & PRAM_BA_STAGE_STEP) {
            const long long most = (long long)F * FC > (long long)P * 3 ? (long long)F * FC : (long long)P * 3;
            hipLaunchKernelGGL(ba_mv_points_kernel<G>, dim3(P), dim3(64), 0, st, g, (const double*)g.x, 1);
            hipLaunchKernelGGL(ba_pose_cand_kernel, per_frame, dim3(256), 0, st, b);
            if constexpr (G::CAM) {
                Ba bc = b;      // the candidate's cost goes through the candidate's parameters
                bc.cam_params = g.cpc;
                hipLaunchKernelGGL(bac_cand_kernel, dim3(cdiv(g.G, 256)), dim3(256), 0, st, g);
                hipLaunchKernelGGL(bac_expand_kernel, dim3(cdiv(F * NK, 256)), dim3(256), 0, st, g, 1);
                hipLaunchKernelGGL(ba_cost_kernel, dim3(F), dim3(256), 0, st, bc, 1);
                hipLaunchKernelGGL(bac_poison_kernel, per_frame, dim3(256), 0, st, g);
            } else {
                hipLaunchKernelGGL(ba_cost_kernel, dim3(F), dim3(256), 0, st, b, 1);
            }
            hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(256), 0, st, b, 0);
            hipLaunchKernelGGL(ba_apply_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, st, b);
            if constexpr (G::CAM) hipLaunchKernelGGL(bac_apply_kernel, dim3(cdiv((F > g.G ? F : g.G) * NK, 256)), dim3(256), 0, st, g);
        }
    }
}

int enqueue_finish(const Ba& g, const char* what, const double* qvec_in, const double* tvec_in, double max_reproj_error, double min_tri_angle,
                   double* qvec, double* tvec, double* xyz, unsigned char* obs_keep, double* obs_error, int* pt_keep, double* pt_error,
                   double* pt_angle, int* pt_kept, int* counts, hipStream_t st) {
    PRAM_REQUIRE(qvec_in && tvec_in && qvec && tvec && xyz && obs_keep && obs_error && pt_keep && pt_error && pt_angle && pt_kept && counts,
                 "%s: null pointer", what);
    PRAM_REQUIRE(aligned(qvec_in, 8) && aligned(tvec_in, 8) && aligned(qvec, 8) && aligned(tvec, 8) && aligned(xyz, 8) && aligned(obs_error, 8) &&
                 aligned(pt_keep, 4) && aligned(pt_error, 8) && aligned(pt_angle, 8) && aligned(pt_kept, 4) && aligned(counts, 4),
                 "%s: misaligned pointer", what);
    PRAM_REQUIRE(max_reproj_error > 0.0 && min_tri_angle >= 0.0, "%s: needs max_reproj_error > 0, min_tri_angle >= 0", what);
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int), st) != hipSuccess) return pram_launch_status(what);
    hipLaunchKernelGGL(ba_filter_obs_kernel, dim3(cdiv(g.n_obs, 256)), dim3(256), 0, st, g, max_reproj_error * max_reproj_error, obs_keep, obs_error,
                       counts);
    hipLaunchKernelGGL(ba_filter_points_kernel, dim3(g.P), dim3(64), 0, st, g, (const unsigned char*)obs_keep, (const double*)obs_error,
                       min_tri_angle, pt_keep, pt_error, pt_angle, pt_kept);
    hipLaunchKernelGGL(ba_poses_out_kernel, dim3(cdiv(g.F, 256)), dim3(256), 0, st, g, qvec_in, tvec_in, qvec, tvec);
    const long long nx = (long long)g.P * 3;
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, (const double*)g.X, xyz, nx);
    return PRAM_OK;
}

}  // namespace

extern "C" size_t pram_ba_workspace_bytes(int n_frames, int n_points, int n_obs, int max_iters) {
    if (!sizes_ok(n_frames, n_points, n_obs, max_iters)) return 0;
    size_t off[A_COUNT + 1];
    layout(n_frames, n_points, n_obs, max_iters, off);
    return off[A_COUNT];
}

extern "C" int pram_ba_layout(int n_frames, int n_points, int n_obs, int max_iters, size_t* offsets) {
    PRAM_REQUIRE(offsets, "pram_ba_layout: null pointer");
    PRAM_REQUIRE(sizes_ok(n_frames, n_points, n_obs, max_iters), "pram_ba_layout: needs 1 <= n_frames <= 2^24, 1 <= n_points <= 2^28, 1 <= n_obs <= 2^26, 0 <= max_iters <= 4096");
    layout(n_frames, n_points, n_obs, max_iters, offsets);
    return PRAM_OK;
}

extern "C" int pram_ba_begin(const float* keypoints, const int* cam_model, const double* cam_params, const int* cam_model_host,
                             const double* table, const double* xyz, const int* obs_row, const int* obs_frame, const int* obs_point,
                             const int* frm_off, const int* pt_off, const int* pt_obs, const int* frozen, int n_frames, int n_points,
                             int n_obs, int n_rows, int max_iters, double loss_scale, double lam0, double cg_tol, double ftol,
                             void* workspace, size_t workspace_bytes, void* context, void* stream) {
    PRAM_REQUIRE(keypoints && cam_model && cam_params && cam_model_host && table && xyz && obs_row && obs_frame && obs_point && frm_off && pt_off &&
                 pt_obs && frozen && workspace && context, "pram_ba_begin: null pointer");
    PRAM_REQUIRE(aligned(keypoints, 4) && aligned(cam_model, 4) && aligned(cam_params, 8) && aligned(table, 8) && aligned(xyz, 8) &&
                 aligned(obs_row, 4) && aligned(obs_frame, 4) && aligned(obs_point, 4) && aligned(frm_off, 4) && aligned(pt_off, 4) &&
                 aligned(pt_obs, 4) && aligned(frozen, 4) && aligned(workspace, 256), "pram_ba_begin: misaligned pointer");
    PRAM_REQUIRE(sizes_ok(n_frames, n_points, n_obs, max_iters) && n_rows >= 1,
                 "pram_ba_begin: needs 1 <= n_frames <= 2^24, 1 <= n_points <= 2^28, 1 <= n_obs <= 2^26, n_rows >= 1, 0 <= max_iters <= 4096");
    PRAM_REQUIRE(loss_scale > 0.0 && isfinite(loss_scale) && lam0 > 0.0 && isfinite(lam0) && cg_tol > 0.0 && cg_tol < 1.0 && ftol >= 0.0 && isfinite(ftol),
                 "pram_ba_begin: needs a finite loss_scale > 0 and lam0 > 0, 0 < cg_tol < 1, a finite ftol >= 0");
    PRAM_REQUIRE(workspace_bytes >= pram_ba_workspace_bytes(n_frames, n_points, n_obs, max_iters), "pram_ba_begin: workspace too small");
    for (int f = 0; f < n_frames; ++f)
        if (cam_model_host[f] < PRAM_CAM_SIMPLE_PINHOLE || cam_model_host[f] > PRAM_CAM_OPENCV) {
            pram_set_error("pram_ba_begin: camera model id %d of frame %d is not supported", cam_model_host[f], f);
            return PRAM_E_UNSUPPORTED;
        }
    size_t off[A_COUNT + 1];
    layout(n_frames, n_points, n_obs, max_iters, off);
    const Ba g = make_base(keypoints, cam_model, cam_params, obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen, n_frames, n_points, n_obs,
                           n_rows, max_iters, static_cast<char*>(workspace), off, MAGIC);
    memset(context, 0, PRAM_BA_CONTEXT_BYTES);
    memcpy(context, &g, sizeof(Ba));
    enqueue_begin(g, table, xyz, loss_scale, lam0, cg_tol, ftol, (hipStream_t)stream);
    return pram_launch_status("pram_ba_begin");
}

extern "C" int pram_ba_iterate(const void* context, int n_iters, int cg_iters, int stages, void* stream) {
    Ba g;
    const int rc = load_ctx(context, &g, "pram_ba_iterate");
    if (rc != PRAM_OK) return rc;
    PRAM_REQUIRE(n_iters >= 0 && n_iters <= MAX_ITERS && cg_iters >= 0 && cg_iters <= 65536 && stages >= 0 && stages <= PRAM_BA_STAGE_ALL,
                 "pram_ba_iterate: needs 0 <= n_iters <= 4096, 0 <= cg_iters <= 65536, 0 <= stages <= PRAM_BA_STAGE_ALL");
    enqueue_iterations(g, n_iters, cg_iters, stages, (hipStream_t)stream);
    return pram_launch_status("pram_ba_iterate");
}

extern "C" int pram_ba_finish(const void* context, const double* qvec_in, const double* tvec_in, double max_reproj_error, double min_tri_angle,
                              double* qvec, double* tvec, double* xyz, unsigned char* obs_keep, double* obs_error, int* pt_keep,
                              double* pt_error, double* pt_angle, int* pt_kept, int* counts, void* stream) {
    Ba g;
    int rc = load_ctx(context, &g, "pram_ba_finish");
    if (rc != PRAM_OK) return rc;
    rc = enqueue_finish(g, "pram_ba_finish", qvec_in, tvec_in, max_reproj_error, min_tri_angle, qvec, tvec, xyz, obs_keep, obs_error, pt_keep, pt_error,
                        pt_angle, pt_kept, counts, (hipStream_t)stream);
    return rc != PRAM_OK ? rc : pram_launch_status("pram_ba_finish");
}

// ---------------------------------------------------------------- the same with camera groups
extern "C" size_t pram_bac_workspace_bytes(int n_frames, int n_points, int n_obs, int n_groups, int max_iters) {
    if (!sizes_cam_ok(n_frames, n_points, n_obs, n_groups, max_iters)) return 0;
    size_t off[C_COUNT + 1];
    layout_cam(n_frames, n_points, n_obs, n_groups, max_iters, off);
    return off[C_COUNT];
}

extern "C" int pram_bac_layout(int n_frames, int n_points, int n_obs, int n_groups, int max_iters, size_t* offsets) {
    PRAM_REQUIRE(offsets, "pram_bac_layout: null pointer");
    PRAM_REQUIRE(sizes_cam_ok(n_frames, n_points, n_obs, n_groups, max_iters), "pram_bac_layout: needs pram_ba_layout's sizes and 1 <= n_groups <= n_frames");
    layout_cam(n_frames, n_points, n_obs, n_groups, max_iters, offsets);
    return PRAM_OK;
}

extern "C" int pram_bac_begin(const float* keypoints, const int* cam_model, const int* cam_model_host, const double* table, const double* xyz,
                              const int* obs_row, const int* obs_frame, const int* obs_point, const int* frm_off, const int* pt_off,
                              const int* pt_obs, const int* frozen, const int* frm_grp, const int* grp_off, const int* grp_frame,
                              const double* grp_params, const int* grp_mask, int n_frames, int n_points, int n_obs, int n_rows, int n_groups,
                              int max_iters, double loss_scale, double lam0, double cg_tol, double ftol, void* workspace, size_t workspace_bytes,
                              void* context, void* stream) {
    PRAM_REQUIRE(keypoints && cam_model && cam_model_host && table && xyz && obs_row && obs_frame && obs_point && frm_off && pt_off && pt_obs &&
                 frozen && frm_grp && grp_off && grp_frame && grp_params && grp_mask && workspace && context, "pram_bac_begin: null pointer");
    PRAM_REQUIRE(aligned(keypoints, 4) && aligned(cam_model, 4) && aligned(table, 8) && aligned(xyz, 8) && aligned(obs_row, 4) &&
                 aligned(obs_frame, 4) && aligned(obs_point, 4) && aligned(frm_off, 4) && aligned(pt_off, 4) && aligned(pt_obs, 4) &&
                 aligned(frozen, 4) && aligned(frm_grp, 4) && aligned(grp_off, 4) && aligned(grp_frame, 4) && aligned(grp_params, 8) &&
                 aligned(grp_mask, 4) && aligned(workspace, 256), "pram_bac_begin: misaligned pointer");
    PRAM_REQUIRE(sizes_cam_ok(n_frames, n_points, n_obs, n_groups, max_iters) && n_rows >= 1,
                 "pram_bac_begin: needs pram_ba_begin's sizes and 1 <= n_groups <= n_frames");
    PRAM_REQUIRE(loss_scale > 0.0 && isfinite(loss_scale) && lam0 > 0.0 && isfinite(lam0) && cg_tol > 0.0 && cg_tol < 1.0 && ftol >= 0.0 && isfinite(ftol),
                 "pram_bac_begin: needs a finite loss_scale > 0 and lam0 > 0, 0 < cg_tol < 1, a finite ftol >= 0");
    PRAM_REQUIRE(workspace_bytes >= pram_bac_workspace_bytes(n_frames, n_points, n_obs, n_groups, max_iters), "pram_bac_begin: workspace too small");
    for (int f = 0; f < n_frames; ++f)
        if (cam_model_host[f] < PRAM_CAM_SIMPLE_PINHOLE || cam_model_host[f] > PRAM_CAM_OPENCV) {
            pram_set_error("pram_bac_begin: camera model id %d of frame %d is not supported", cam_model_host[f], f);
            return PRAM_E_UNSUPPORTED;
        }
    size_t off[C_COUNT + 1];
    layout_cam(n_frames, n_points, n_obs, n_groups, max_iters, off);
    char* w = static_cast<char*>(workspace);
    const auto D = [&](int a) { return reinterpret_cast<double*>(w + off[a]); };
    const auto I = [&](int a) { return reinterpret_cast<int*>(w + off[a]); };
    Bac g;
    static_cast<Ba&>(g) = make_base(keypoints, cam_model, D(C_CP), obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen, n_frames, n_points,
                                    n_obs, n_rows, max_iters, w, off, MAGIC_CAM);
    g.frm_grp = frm_grp; g.grp_off = grp_off; g.grp_frame = grp_frame; g.grp_mask_in = grp_mask; g.grp_params_in = grp_params; g.G = n_groups;
    g.cp = D(C_CP); g.cpc = D(C_CPC); g.k = D(C_K); g.kc = D(C_KC); g.Sg = D(C_SG); g.dUg = D(C_DUG); g.bg = D(C_BG); g.gx = D(C_GX); g.gr = D(C_GR);
    g.gz = D(C_GZ); g.gpv = D(C_GP); g.gq = D(C_GQ); g.gdot = D(C_GDOT); g.gpart = D(C_GPART); g.fpart = D(C_FPART); g.mvpart = D(C_MVPART);
    g.gmask = I(C_GMASK); g.gbad = I(C_GBAD); g.gmodel = I(C_GMODEL); g.gfold = D(C_GFOLD);
    memset(context, 0, PRAM_BAC_CONTEXT_BYTES);
    memcpy(context, static_cast<const void*>(&g), sizeof(Bac));
    enqueue_begin(g, table, xyz, loss_scale, lam0, cg_tol, ftol, (hipStream_t)stream);
    return pram_launch_status("pram_bac_begin");
}

extern "C" int pram_bac_iterate(const void* context, int n_iters, int cg_iters, int stages, void* stream) {
    Bac g;
    const int rc = load_ctx_cam(context, &g, "pram_bac_iterate");
    if (rc != PRAM_OK) return rc;
    PRAM_REQUIRE(n_iters >= 0 && n_iters <= MAX_ITERS && cg_iters >= 0 && cg_iters <= 65536 && stages >= 0 && stages <= PRAM_BA_STAGE_ALL,
                 "pram_bac_iterate: needs 0 <= n_iters <= 4096, 0 <= cg_iters <= 65536, 0 <= stages <= PRAM_BA_STAGE_ALL");
    enqueue_iterations(g, n_iters, cg_iters, stages, (hipStream_t)stream);
    return pram_launch_status("pram_bac_iterate");
}

extern "C" int pram_bac_finish(const void* context, const double* qvec_in, const double* tvec_in, double max_reproj_error, double min_tri_angle,
                               double* qvec, double* tvec, double* xyz, unsigned char* obs_keep, double* obs_error, int* pt_keep,
                               double* pt_error, double* pt_angle, int* pt_kept, int* counts, double* grp_params, void* stream) {
    Bac g;
    int rc = load_ctx_cam(context, &g, "pram_bac_finish");
    if (rc != PRAM_OK) return rc;
    PRAM_REQUIRE(grp_params && aligned(grp_params, 8), "pram_bac_finish: grp_params is null or misaligned");
    hipStream_t st = (hipStream_t)stream;
    rc = enqueue_finish(g, "pram_bac_finish", qvec_in, tvec_in, max_reproj_error, min_tri_angle, qvec, tvec, xyz, obs_keep, obs_error, pt_keep, pt_error,
                        pt_angle, pt_kept, counts, st);
    if (rc != PRAM_OK) return rc;
    // the accepted parameters: a group that never moved still holds its input bit for bit.  Tables that failed the check: the input
    const long long nk = (long long)g.G * NK;
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, g.grp_params_in, grp_params, nk);
    hipLaunchKernelGGL(bac_params_out_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, g, grp_params);
    return pram_launch_status("pram_bac_finish");
}
