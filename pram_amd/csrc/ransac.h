// What the RANSAC stages share (pose.hip, twoview.hip): the ranking rule and the kernel that picks a pair's best slot by it, the
// 6 x 6 damped Cholesky of the Levenberg-Marquardt step, the pose (Pose) with its rotation update and finiteness test, the
// Levenberg-Marquardt driver of a workgroup (LmState, lm_refine) and the rotation-to-quaternion conversion.  bundle.hip takes the
// Cholesky, the conversion and the pose tangent (Pose, pose_update) from here.
#pragma once
#include "camera.h"

// better(a, b): most inliers, then smaller residual sum, then smaller index
__device__ __forceinline__ bool better(int ca, double ra, int ia, int cb, double rb, int ib) {
    if (ca != cb) return ca > cb;
    if (ra != rb) return ra < rb;
    return ia < ib;
}

// one workgroup per pair: the best slot by the ranking rule (-1 if no slot holds a hypothesis)
static __global__ __launch_bounds__(256) void ransac_pick_kernel(const int* __restrict__ h_inl, const double* __restrict__ h_res, int slots,
                                                        int* __restrict__ best) {
    __shared__ int sc[4], si[4];
    __shared__ double sr[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* hc = h_inl + (size_t)p * slots;
    const double* hr = h_res + (size_t)p * slots;
    int bc = -1, bi = 0x7fffffff;
    double br = 0.0;
    for (int i = tid; i < slots; i += 256) {
        const int c = hc[i];
        const double r = hr[i];
        if (c >= 0 && better(c, r, i, bc, br, bi)) { bc = c; br = r; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o, 64), oi = __shfl_xor(bi, o, 64);
        const double orr = __shfl_xor(br, o, 64);
        if (oc >= 0 && better(oc, orr, oi, bc, br, bi)) { bc = oc; br = orr; bi = oi; }
    }
    if (lane == 0) { sc[wave] = bc; sr[wave] = br; si[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (sc[w] >= 0 && better(sc[w], sr[w], si[w], bc, br, bi)) { bc = sc[w]; br = sr[w]; bi = si[w]; }
        best[p] = bc >= 0 ? bi : -1;
    }
}

// (H + lam diag(H)) x = -g by Cholesky; false when a pivot is not positive or the step is not finite.  H: 21 upper-triangle values.
static __device__ bool chol_solve6(const double* __restrict__ Hu, const double* __restrict__ g, double lam, double* x) {
    double M[6][6], L[6][6];
    int e = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) { M[a][c] = Hu[e]; M[c][a] = Hu[e]; ++e; }
    for (int a = 0; a < 6; ++a) M[a][a] = M[a][a] + lam * M[a][a];
    for (int i = 0; i < 6; ++i)
        for (int k = 0; k <= i; ++k) {
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += L[i][j] * L[k][j];
            s = M[i][k] - s;
            if (i == k) {
                if (!(s > 0.0)) return false;
                L[i][i] = sqrt(s);
            } else {
                L[i][k] = s / L[k][k];
            }
        }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double s = 0.0;
        for (int j = 0; j < i; ++j) s += L[i][j] * y[j];
        y[i] = (-g[i] - s) / L[i][i];
    }
    bool okx = true;
    for (int i = 5; i >= 0; --i) {
        double s = 0.0;
        for (int j = i + 1; j < 6; ++j) s += L[j][i] * x[j];
        x[i] = (y[i] - s) / L[i][i];
        okx = okx && fin(x[i]);
    }
    return okx;
}

// A rigid motion x -> R x + t, R row-major: an absolute pose (pose.hip, bundle.hip) or a relative one (twoview.hip, |t| = 1)
struct Pose { double R[9], t[3]; };

__device__ __forceinline__ bool pose_finite(const Pose& q) {
    bool okq = true;
    for (int a = 0; a < 9; ++a) okq = okq && fin(q.R[a]);
    for (int a = 0; a < 3; ++a) okq = okq && fin(q.t[a]);
    return okq;
}

// out = exp([d]x) R by Rodrigues' formula on d[0 .. 3), first order below |d| = 1e-12
static __device__ void rot_exp_left(const double* __restrict__ d, const double* __restrict__ R, double* __restrict__ out) {
    const double th = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    double E[9];
    if (th < 1e-12) {
        E[0] = 1.0; E[1] = -d[2]; E[2] = d[1]; E[3] = d[2]; E[4] = 1.0; E[5] = -d[0]; E[6] = -d[1]; E[7] = d[0]; E[8] = 1.0;
    } else {
        const double kx = d[0] / th, ky = d[1] / th, kz = d[2] / th;
        const double K[9] = {0.0, -kz, ky, kz, 0.0, -kx, -ky, kx, 0.0};
        const double sn = sin(th), cs = 1.0 - cos(th);
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) {
                const double kk = K[a * 3] * K[c] + K[a * 3 + 1] * K[3 + c] + K[a * 3 + 2] * K[6 + c];
                E[a * 3 + c] = (a == c ? 1.0 : 0.0) + sn * K[a * 3 + c] + cs * kk;
            }
    }
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) out[a * 3 + c] = E[a * 3] * R[c] + E[a * 3 + 1] * R[3 + c] + E[a * 3 + 2] * R[6 + c];
}

// the pose tangent of the Levenberg-Marquardt steps (pose.hip, bundle.hip): R <- exp([w]x) R, t <- t + d
static __device__ void pose_update(const Pose& q, const double* __restrict__ d, Pose& o) {
    rot_exp_left(d, q.R, o.R);
    o.t[0] = q.t[0] + d[3]; o.t[1] = q.t[1] + d[4]; o.t[2] = q.t[2] + d[5];
}

// The Levenberg-Marquardt driver of one workgroup of 256 threads over NV sums (cost first, then H and g as the model lays them
// out).  The state lives in LDS; wred and tot are block_fold_f64's.
constexpr double LM_LAMBDA0 = 1e-3;

template <class Model, int NV>
struct LmState {
    double wred[4][NV];
    double tot[NV];
    double cur[NV];      // cost, H, g at the accepted model
    Model cand;
    int solved;
};

// `iters` iterations from q; every thread calls it with the same q and ends with the same model.  pass(m) is called by every
// thread and leaves cost, H, g at m in sh.tot, readable by every thread (it ends in block_fold_f64); step(cur, lam, q, cand) runs
// on thread 0 alone, solves the damped system at the accepted sums `cur` and writes the candidate, false when there is none.
template <class Model, int NV, class Pass, class Step>
__device__ __forceinline__ void lm_refine(Model& q, int iters, LmState<Model, NV>& sh, Pass pass, Step step) {
    const int tid = threadIdx.x;
    pass(q);
    if (tid < NV) sh.cur[tid] = sh.tot[tid];
    double lam = LM_LAMBDA0;
    for (int it = 0; it < iters; ++it) {
        __syncthreads();      // cur is complete, solved / cand of the previous iteration have been read
        if (tid == 0) sh.solved = step(sh.cur, lam, q, sh.cand);
        __syncthreads();
        if (!sh.solved) { lam *= 10.0; continue; }      // uniform over the workgroup
        const Model c = sh.cand;
        pass(c);
        const bool accept = sh.tot[0] < sh.cur[0];      // NaN compares false: rejected
        __syncthreads();
        if (accept) {
            q = c;
            if (tid < NV) sh.cur[tid] = sh.tot[tid];
            lam = fmax(lam * 0.1, 1e-15);
        } else {
            lam *= 10.0;
        }
    }
    __syncthreads();
}

static __device__ void rot_to_qvec(const double* __restrict__ R, double* __restrict__ qv) {
    const double tr = R[0] + R[4] + R[8];
    double q0, q1, q2, q3;
    if (tr > 0.0) {
        const double s = sqrt(tr + 1.0) * 2.0;
        q0 = 0.25 * s; q1 = (R[7] - R[5]) / s; q2 = (R[2] - R[6]) / s; q3 = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
        q0 = (R[7] - R[5]) / s; q1 = 0.25 * s; q2 = (R[1] + R[3]) / s; q3 = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
        q0 = (R[2] - R[6]) / s; q1 = (R[1] + R[3]) / s; q2 = 0.25 * s; q3 = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
        q0 = (R[3] - R[1]) / s; q1 = (R[2] + R[6]) / s; q2 = (R[5] + R[7]) / s; q3 = 0.25 * s;
    }
    const double nrm = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double sg = q0 / nrm < 0.0 ? -1.0 : 1.0;
    qv[0] = sg * (q0 / nrm); qv[1] = sg * (q1 / nrm); qv[2] = sg * (q2 / nrm); qv[3] = sg * (q3 / nrm);
}
