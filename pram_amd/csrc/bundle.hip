// Global bundle adjustment of a map on the device: the frames' poses (cam_from_world) and the points, jointly, under the robust
// cost of pose.hip (s = |r|^2 / loss_scale^2, cost log1p(s), weight 1 / (1 + s)), intrinsics constant.  Levenberg-Marquardt; the
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
__global__ __launch_bounds__(256) void ba_linearise_kernel(Ba g) {
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
        for (int k = 0; k < 3; ++k) out[12 + i * 3 + k] = sw * jp[k];
    }
    out[18] = sw * r0; out[19] = sw * r1;
}

// ---------------------------------------------------------------- blocks
// one wave per point: V = sum J_p^T J_p, g_p, the inverse of V + lam diag(V) by chol_solve3
__global__ __launch_bounds__(64) void ba_points_kernel(Ba g) {
    if (g.si[SI_DONE]) return;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int beg = g.pt_off[p], end = g.pt_off[p + 1];
    double acc[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = 0.0;
    int cnt = 0;
    for (int k = beg + lane; k < end; k += 64) {
        const int o = g.pt_obs[k];
        const double* j = g.J + (size_t)o * JW + 12;
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

// one workgroup per frame: U, g_c, the frame's diagonal block of S = U - W V^-1 W^T and b = W V^-1 g_p - g_c
__global__ __launch_bounds__(256) void ba_frames_kernel(Ba g) {
    __shared__ double wred[4][NV_FRAME], tot[NV_FRAME];
    if (g.si[SI_DONE]) return;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int beg = g.frm_off[f], end = g.frm_off[f + 1];
    double acc[NV_FRAME];
#pragma unroll
    for (int e = 0; e < NV_FRAME; ++e) acc[e] = 0.0;
    for (int o = beg + tid; o < end; o += 256) {
        const double* j = g.J + (size_t)o * JW;
        const int p = g.obs_point[o];
        const double* V = g.Vinv + (size_t)p * 6;
        const double* gp = g.gp + (size_t)p * 3;
        double jc[12], jp[6];
#pragma unroll
        for (int e = 0; e < 12; ++e) jc[e] = j[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) jp[e] = j[12 + e];
        const double r0 = j[18], r1 = j[19];
        double W[6][3], WV[6][3];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int k = 0; k < 3; ++k) W[a][k] = jc[a] * jp[k] + jc[6 + a] * jp[3 + k];
            vinv_mul(V, W[a], WV[a]);
        }
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) {
                const double u = jc[a] * jc[c] + jc[6 + a] * jc[6 + c];
                const double w = WV[a][0] * W[c][0] + WV[a][1] * W[c][1] + WV[a][2] * W[c][2];
                acc[e++] += u - w;
            }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            acc[21 + a] += jc[a] * jc[a] + jc[6 + a] * jc[6 + a];
            acc[27 + a] += jc[a] * r0 + jc[6 + a] * r1;
            acc[33 + a] += WV[a][0] * gp[0] + WV[a][1] * gp[1] + WV[a][2] * gp[2];
        }
    }
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

// ---------------------------------------------------------------- conjugate gradients on S d_c = b
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

__global__ __launch_bounds__(256) void ba_cg_start_kernel(Ba g) {
    __shared__ double sh[1];
    if (g.si[SI_DONE]) return;
    const int nb = cdiv_d(g.F, BLK);
    const double rz = blocked_sum(g.fdot, g.F, g.part, sh), bb = blocked_sum(g.fdot + g.F, g.F, g.part + nb, sh);
    if (threadIdx.x == 0) {
        g.sd[SD_RZ] = rz; g.sd[SD_BB] = bb; g.sd[SD_RR] = bb;
        if (!(bb > 0.0)) g.si[SI_CG_DONE] = 1;      // b = 0 (or not a number): d_c = 0
    }
}

// one wave per point.  mode 0: y_p = V^-1 sum J_p^T J_c v_c (the first pass of a matvec); mode 1: the back-substitution
// d_p = -V^-1 (g_p + sum J_p^T J_c d_c) and the candidate point
__global__ __launch_bounds__(64) void ba_mv_points_kernel(Ba g, const double* __restrict__ vec, int mode) {
    if (g.si[SI_DONE] || (mode == 0 && g.si[SI_CG_DONE])) return;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int beg = g.pt_off[p], end = g.pt_off[p + 1];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = beg + lane; k < end; k += 64) {
        const int o = g.pt_obs[k];
        const double* j = g.J + (size_t)o * JW;
        const double* v = vec + (size_t)g.obs_frame[o] * 6;
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { t0 += j[a] * v[a]; t1 += j[6 + a] * v[a]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += j[12 + c] * t0 + j[15 + c] * t1;
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
__global__ __launch_bounds__(256) void ba_mv_frames_kernel(Ba g) {
    __shared__ double wred[4][6], tot[6];
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int beg = g.frm_off[f], end = g.frm_off[f + 1];
    double v[6], acc[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) { v[a] = g.p[(size_t)f * 6 + a]; acc[a] = 0.0; }
    for (int o = beg + tid; o < end; o += 256) {
        const double* j = g.J + (size_t)o * JW;
        const double* y = g.yp + (size_t)g.obs_point[o] * 3;
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { t0 += j[a] * v[a]; t1 += j[6 + a] * v[a]; }
        t0 -= j[12] * y[0] + j[13] * y[1] + j[14] * y[2];
        t1 -= j[15] * y[0] + j[16] * y[1] + j[17] * y[2];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] += j[a] * t0 + j[6 + a] * t1;
    }
    block_fold_f64<6>(acc, wred, tot);
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

__global__ __launch_bounds__(256) void ba_cg_alpha_kernel(Ba g) {
    __shared__ double sh[1];
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const double pap = blocked_sum(g.fdot, g.F, g.part, sh);
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

__global__ __launch_bounds__(256) void ba_cg_beta_kernel(Ba g) {
    __shared__ double sh[1];
    if (g.si[SI_DONE] || g.si[SI_CG_DONE]) return;
    const int nb = cdiv_d(g.F, BLK);
    const double rz = blocked_sum(g.fdot, g.F, g.part, sh), rr = blocked_sum(g.fdot + g.F, g.F, g.part + nb, sh);
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

// offsets [PRAM_BA_ARRAYS + 1] of the workspace's arrays, the last one the total
void layout(int F, int P, int n_obs, int max_iters, size_t* off) {
    const size_t d = sizeof(double), i = sizeof(int), nb = (size_t)cdiv(F, BLK);
    const size_t bytes[A_COUNT] = {(size_t)F * FC * d, (size_t)F * FC * d, (size_t)P * 3 * d, (size_t)P * 3 * d, (size_t)n_obs * JW * d, (size_t)P * 6 * d,
                                   (size_t)P * 3 * d, (size_t)P * 3 * d, (size_t)F * 21 * d, (size_t)F * 6 * d, (size_t)F * 6 * d, (size_t)F * 6 * d,
                                   (size_t)F * 6 * d, (size_t)F * 6 * d, (size_t)F * 6 * d, (size_t)F * 6 * d, (size_t)F * 2 * d, (size_t)F * d, 2 * nb * d,
                                   (size_t)PRAM_BA_STATE_F64 * d, (size_t)(PRAM_BA_STATE_I32 + 2 * max_iters) * i, (size_t)P * i, (size_t)F * i,
                                   (size_t)F * i, (size_t)n_obs};
    off[0] = 0;
    for (int a = 0; a < A_COUNT; ++a) off[a + 1] = off[a] + al(bytes[a]);
}

int load_ctx(const void* ctx, Ba* g, const char* what) {
    PRAM_REQUIRE(ctx, "%s: null context", what);
    memcpy(g, ctx, sizeof(Ba));
    PRAM_REQUIRE(g->magic == MAGIC, "%s: the context is not one pram_ba_begin filled", what);
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
    char* w = static_cast<char*>(workspace);
    const auto D = [&](int a) { return reinterpret_cast<double*>(w + off[a]); };
    const auto I = [&](int a) { return reinterpret_cast<int*>(w + off[a]); };
    Ba g = {keypoints, cam_model, cam_params, obs_row, obs_frame, obs_point, frm_off, pt_off, pt_obs, frozen, n_frames, n_points, n_obs, n_rows,
            max_iters, D(A_T), D(A_TC), D(A_X), D(A_XC), D(A_J), D(A_VINV), D(A_GP), D(A_YP), D(A_SBLK), D(A_DU), D(A_B), D(A_CGX), D(A_CGR),
            D(A_CGZ), D(A_CGP), D(A_CGQ), D(A_FDOT), D(A_FCOST), D(A_PART), D(A_SD), I(A_SI), I(A_PFLAG), I(A_MOVED), I(A_FMASK),
            reinterpret_cast<unsigned char*>(w + off[A_OOK]), MAGIC};
    memset(context, 0, PRAM_BA_CONTEXT_BYTES);
    memcpy(context, &g, sizeof(Ba));
    hipStream_t st = (hipStream_t)stream;
    const int F = n_frames, P = n_points;
    const int most = n_obs > F ? (n_obs > P ? n_obs : P) : (F > P ? F : P);
    hipLaunchKernelGGL(ba_init_kernel, dim3(1), dim3(1), 0, st, g, loss_scale, lam0, cg_tol, ftol);
    hipLaunchKernelGGL(ba_check_kernel, dim3(cdiv(most, 256)), dim3(256), 0, st, g);
    const long long nt = (long long)F * FC, nx = (long long)P * 3;
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, table, g.T, nt);
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, table, g.Tc, nt);
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, xyz, g.X, nx);
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, xyz, g.Xc, nx);
    hipLaunchKernelGGL(ba_cost_kernel, dim3(F), dim3(256), 0, st, g, 0);
    hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(256), 0, st, g, 1);
    return pram_launch_status("pram_ba_begin");
}

extern "C" int pram_ba_iterate(const void* context, int n_iters, int cg_iters, int stages, void* stream) {
    Ba g;
    const int rc = load_ctx(context, &g, "pram_ba_iterate");
    if (rc != PRAM_OK) return rc;
    PRAM_REQUIRE(n_iters >= 0 && n_iters <= MAX_ITERS && cg_iters >= 0 && cg_iters <= 65536 && stages >= 0 && stages <= PRAM_BA_STAGE_ALL,
                 "pram_ba_iterate: needs 0 <= n_iters <= 4096, 0 <= cg_iters <= 65536, 0 <= stages <= PRAM_BA_STAGE_ALL");
    hipStream_t st = (hipStream_t)stream;
    const int F = g.F, P = g.P;
    const dim3 per_frame(cdiv(F, 256)), per_unknown(cdiv(F * 6, 256));
    for (int it = 0; it < n_iters; ++it) {
        if (stages & PRAM_BA_STAGE_LINEARISE) hipLaunchKernelGGL(ba_linearise_kernel, dim3(cdiv(g.n_obs, 256)), dim3(256), 0, st, g);
        if (stages & PRAM_BA_STAGE_BLOCKS) {
            hipLaunchKernelGGL(ba_points_kernel, dim3(P), dim3(64), 0, st, g);
            hipLaunchKernelGGL(ba_frames_kernel, dim3(F), dim3(256), 0, st, g);
        }
        if (stages & PRAM_BA_STAGE_CG_INIT) {
            hipLaunchKernelGGL(ba_cg_init_kernel, per_frame, dim3(256), 0, st, g);
            hipLaunchKernelGGL(ba_cg_start_kernel, dim3(1), dim3(256), 0, st, g);
        }
        if (stages & PRAM_BA_STAGE_CG)
            for (int k = 0; k < cg_iters; ++k) {
                hipLaunchKernelGGL(ba_mv_points_kernel, dim3(P), dim3(64), 0, st, g, (const double*)g.p, 0);
                hipLaunchKernelGGL(ba_mv_frames_kernel, dim3(F), dim3(256), 0, st, g);
                hipLaunchKernelGGL(ba_cg_alpha_kernel, dim3(1), dim3(256), 0, st, g);
                hipLaunchKernelGGL(ba_cg_update_kernel, per_frame, dim3(256), 0, st, g);
                hipLaunchKernelGGL(ba_cg_beta_kernel, dim3(1), dim3(256), 0, st, g);
                hipLaunchKernelGGL(ba_cg_dir_kernel, per_unknown, dim3(256), 0, st, g);
            }
        if (stages & PRAM_BA_STAGE_STEP) {
            const long long most = (long long)F * FC > (long long)P * 3 ? (long long)F * FC : (long long)P * 3;
            hipLaunchKernelGGL(ba_mv_points_kernel, dim3(P), dim3(64), 0, st, g, (const double*)g.x, 1);
            hipLaunchKernelGGL(ba_pose_cand_kernel, per_frame, dim3(256), 0, st, g);
            hipLaunchKernelGGL(ba_cost_kernel, dim3(F), dim3(256), 0, st, g, 1);
            hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(256), 0, st, g, 0);
            hipLaunchKernelGGL(ba_apply_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, st, g);
        }
    }
    return pram_launch_status("pram_ba_iterate");
}

extern "C" int pram_ba_finish(const void* context, const double* qvec_in, const double* tvec_in, double max_reproj_error, double min_tri_angle,
                              double* qvec, double* tvec, double* xyz, unsigned char* obs_keep, double* obs_error, int* pt_keep,
                              double* pt_error, double* pt_angle, int* pt_kept, int* counts, void* stream) {
    Ba g;
    const int rc = load_ctx(context, &g, "pram_ba_finish");
    if (rc != PRAM_OK) return rc;
    PRAM_REQUIRE(qvec_in && tvec_in && qvec && tvec && xyz && obs_keep && obs_error && pt_keep && pt_error && pt_angle && pt_kept && counts,
                 "pram_ba_finish: null pointer");
    PRAM_REQUIRE(aligned(qvec_in, 8) && aligned(tvec_in, 8) && aligned(qvec, 8) && aligned(tvec, 8) && aligned(xyz, 8) && aligned(obs_error, 8) &&
                 aligned(pt_keep, 4) && aligned(pt_error, 8) && aligned(pt_angle, 8) && aligned(pt_kept, 4) && aligned(counts, 4),
                 "pram_ba_finish: misaligned pointer");
    PRAM_REQUIRE(max_reproj_error > 0.0 && min_tri_angle >= 0.0, "pram_ba_finish: needs max_reproj_error > 0, min_tri_angle >= 0");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int), st) != hipSuccess) return pram_launch_status("pram_ba_finish");
    hipLaunchKernelGGL(ba_filter_obs_kernel, dim3(cdiv(g.n_obs, 256)), dim3(256), 0, st, g, max_reproj_error * max_reproj_error, obs_keep, obs_error,
                       counts);
    hipLaunchKernelGGL(ba_filter_points_kernel, dim3(g.P), dim3(64), 0, st, g, (const unsigned char*)obs_keep, (const double*)obs_error,
                       min_tri_angle, pt_keep, pt_error, pt_angle, pt_kept);
    hipLaunchKernelGGL(ba_poses_out_kernel, dim3(cdiv(g.F, 256)), dim3(256), 0, st, g, qvec_in, tvec_in, qvec, tvec);
    const long long nx = (long long)g.P * 3;
    hipLaunchKernelGGL(ba_copy_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, (const double*)g.X, xyz, nx);
    return pram_launch_status("pram_ba_finish");
}
