// Batched absolute pose from the 2D-3D matches of pram_cand_correspond (what SingleMap3D.localize_with_ref_frame hands to
// pycolmap.absolute_pose_estimation, singlemap3d.py:168-193, and the candidate loop's verify_and_update, multimap3d.py:183-239,
// 294-313): P3P RANSAC with a fixed trial budget, Levenberg-Marquardt refinement and the choice among the seg_k candidates of a
// query, for all pairs at once.  float64 throughout (world coordinates of hundreds of metres; the P3P quartic is ill-conditioned
// in fp32).  Every loop has a compile-time or argument-given bound.  DESIGN.md 4.12 has the layout and the formulas.
#include "camera.h"
#include "ransac.h"
#include <math.h>

namespace {

constexpr int UNDISTORT_STEPS = PRAM_POSE_UNDISTORT_STEPS;
constexpr int CUBIC_POLISH = 2;
constexpr int QUARTIC_POLISH = 3;
constexpr int SCORE_CHUNK = 768;          // rows per LDS chunk: 5 doubles each = 30 KB (always chunked, whatever t0)
constexpr int SCORE_TPW = 4;              // trials a wave takes in turn on every chunk
constexpr int SCORE_TRIALS = 4 * SCORE_TPW;      // trials per workgroup: the rows staged in LDS serve 16 trials = 64 slots

// ---------------------------------------------------------------- prepare: pixels -> normalised camera plane
__global__ __launch_bounds__(256) void pose_prepare_kernel(const float* __restrict__ kpts, const int* __restrict__ count,
                                                           const int* __restrict__ cam_model, const double* __restrict__ cam_params,
                                                           int seg_k, int t0, double* __restrict__ pts) {
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    int n = count[p];
    n = n > t0 ? t0 : n;
    if (i >= n) return;
    const int b = p / seg_k;
    const Cam c = cam_unify(cam_model[b], cam_params + (size_t)b * PRAM_POSE_CAM_PARAMS);
    const size_t row = (size_t)p * t0 + i;
    const double xd = (((double)kpts[row * 2] + 0.5) - c.cx) / c.fx, yd = (((double)kpts[row * 2 + 1] + 0.5) - c.cy) / c.fy;
    double u = xd, v = yd;
    for (int it = 0; it < UNDISTORT_STEPS; ++it) {
        double fu, fv, j11, j12, j22;
        distort(c, u, v, fu, fv);
        fu -= xd; fv -= yd;
        distort_jac(c, u, v, j11, j12, j22);
        const double det = j11 * j22 - j12 * j12;
        if (fabs(det) > 1e-12) {
            const double su = (j22 * fu - j12 * fv) / det, sv = (j11 * fv - j12 * fu) / det;
            u -= su; v -= sv;
        }
    }
    pts[row * 2] = u; pts[row * 2 + 1] = v;
}

// ---------------------------------------------------------------- hypotheses: sampler + P3P (Grunert's quartic)
__device__ __forceinline__ V3 scale(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 divs(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }

__device__ __forceinline__ V3 bearing(const double* __restrict__ pt) {
    const double x = pt[0], y = pt[1];
    const double nrm = sqrt(x * x + y * y + 1.0);
    return {x / nrm, y / nrm, 1.0 / nrm};
}

__global__ __launch_bounds__(256) void pose_hypotheses_kernel(const double* __restrict__ pts, const double* __restrict__ xyz,
                                                              const int* __restrict__ count, int t0, int trials, unsigned long long seed,
                                                              double* __restrict__ poses, int* __restrict__ n_sol, int* __restrict__ triples) {
    const int p = blockIdx.y, tr = blockIdx.x * 256 + threadIdx.x;
    if (tr >= trials) return;
    const size_t slot = (size_t)p * trials + tr;
    double* out = poses + slot * 48;
    int n = count[p];
    n = n > t0 ? t0 : n;
    int i0 = -1, i1 = -1, i2 = -1, ns = 0;
    double sol[4][12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 12; ++e) sol[k][e] = 0.0;
    if (n >= 3) {
        const unsigned long long key = sm64(sm64(seed) ^ (((unsigned long long)(unsigned)p << 32) | (unsigned long long)(unsigned)tr));
        i0 = (int)__umul64hi(sm64(key + 0ull), (unsigned long long)n);
        i1 = (int)__umul64hi(sm64(key + 1ull), (unsigned long long)(n - 1));
        i2 = (int)__umul64hi(sm64(key + 2ull), (unsigned long long)(n - 2));
        i1 += i1 >= i0;
        const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
        i2 += i2 >= lo;
        i2 += i2 >= hi;
        const double* pb = pts + (size_t)p * t0 * 2;
        const double* xb = xyz + (size_t)p * t0 * 3;
        const V3 j1 = bearing(pb + (size_t)i0 * 2), j2 = bearing(pb + (size_t)i1 * 2), j3 = bearing(pb + (size_t)i2 * 2);
        const V3 P1 = {xb[(size_t)i0 * 3], xb[(size_t)i0 * 3 + 1], xb[(size_t)i0 * 3 + 2]};
        const V3 P2 = {xb[(size_t)i1 * 3], xb[(size_t)i1 * 3 + 1], xb[(size_t)i1 * 3 + 2]};
        const V3 P3 = {xb[(size_t)i2 * 3], xb[(size_t)i2 * 3 + 1], xb[(size_t)i2 * 3 + 2]};
        const V3 d12 = sub(P2, P1), d13 = sub(P3, P1), d23 = sub(P3, P2);
        const double a2 = dot(d23, d23), b2 = dot(d13, d13), c2 = dot(d12, d12);
        const V3 cr = cross(d12, d13);
        const double cr2 = dot(cr, cr);
        if (cr2 > 1e-18 * c2 * b2) {      // not collinear, no duplicate (NaN compares false)
            const double ca = dot(j2, j3), cb = dot(j1, j3), cg = dot(j1, j2);
            const double K = (a2 - c2) / b2, cr_ = c2 / b2;
            const double n2 = K - 1.0, n1 = -2.0 * K * cb, n0 = 1.0 + K;
            const double e1 = -2.0 * ca, e0 = 2.0 * cg;
            const double q2 = -cr_, q1 = 2.0 * cr_ * cb, q0 = 1.0 - cr_;
            const double dd2 = e1 * e1, dd1 = 2.0 * e1 * e0, dd0 = e0 * e0;
            const double A4 = n2 * n2 + dd2 * q2;
            const double A3 = 2.0 * n2 * n1 + (dd2 * q1 + dd1 * q2) - e0 * (n2 * e1);
            const double A2 = (2.0 * n2 * n0 + n1 * n1) + (dd2 * q0 + dd1 * q1 + dd0 * q2) - e0 * (n2 * e0 + n1 * e1);
            const double A1 = 2.0 * n1 * n0 + (dd1 * q0 + dd0 * q1) - e0 * (n1 * e0 + n0 * e1);
            const double A0 = n0 * n0 + dd0 * q0 - e0 * (n0 * e0);
            // Ferrari: monic, depressed, the largest root of the resolvent cubic, two quadratics
            const double b = A3 / A4, c = A2 / A4, d = A1 / A4, e = A0 / A4;
            const double pp = c - 0.375 * b * b;
            const double q = d - 0.5 * b * c + 0.125 * b * b * b;
            const double r = e - 0.25 * b * d + 0.0625 * b * b * c - 0.01171875 * b * b * b * b;
            const double c2_ = pp, c1_ = 0.25 * (pp * pp - 4.0 * r), c0_ = -0.125 * q * q;
            const double Qc = (c2_ * c2_ - 3.0 * c1_) / 9.0;
            const double Rc = (2.0 * c2_ * c2_ * c2_ - 9.0 * c2_ * c1_ + 27.0 * c0_) / 54.0;
            const double Q3 = Qc * Qc * Qc;
            double m;
            if (Rc * Rc < Q3) {
                double ratio = Rc / sqrt(Q3);
                ratio = ratio < -1.0 ? -1.0 : (ratio > 1.0 ? 1.0 : ratio);
                const double th = acos(ratio), sq = -2.0 * sqrt(Qc);
                const double TWO_PI = 2.0 * 3.141592653589793;
                m = fmax(fmax(sq * cos(th / 3.0), sq * cos((th + TWO_PI) / 3.0)), sq * cos((th - TWO_PI) / 3.0));
            } else {
                const double sg = Rc > 0.0 ? 1.0 : (Rc < 0.0 ? -1.0 : 0.0);
                const double A = -sg * cbrt(fabs(Rc) + sqrt(Rc * Rc - Q3));
                const double B = A != 0.0 ? Qc / A : 0.0;
                m = A + B;
            }
            m = m - c2_ / 3.0;
            for (int it = 0; it < CUBIC_POLISH; ++it) {
                const double g = ((m + c2_) * m + c1_) * m + c0_;
                const double dg = (3.0 * m + 2.0 * c2_) * m + c1_;
                if (dg != 0.0) m = m - g / dg;
            }
            double y[4];
            bool ok[4];
            if (m > 0.0) {
                const double s = sqrt(2.0 * m), h = 0.5 * pp + m, g = q / (2.0 * s);
                const double D1 = s * s - 4.0 * (h + g), D2 = s * s - 4.0 * (h - g);
                const double r1 = sqrt(fmax(D1, 0.0)), r2 = sqrt(fmax(D2, 0.0));
                y[0] = 0.5 * (s + r1); y[1] = 0.5 * (s - r1); y[2] = 0.5 * (-s + r2); y[3] = 0.5 * (-s - r2);
                ok[0] = ok[1] = D1 >= 0.0; ok[2] = ok[3] = D2 >= 0.0;
            } else {      // q = 0: a biquadratic
                const double db = pp * pp - 4.0 * r;
                const double rb = sqrt(fmax(db, 0.0));
                const double z1 = 0.5 * (-pp + rb), z2 = 0.5 * (-pp - rb);
                const double w1 = sqrt(fmax(z1, 0.0)), w2 = sqrt(fmax(z2, 0.0));
                y[0] = w1; y[1] = -w1; y[2] = w2; y[3] = -w2;
                ok[0] = ok[1] = db >= 0.0 && z1 >= 0.0; ok[2] = ok[3] = db >= 0.0 && z2 >= 0.0;
            }
            // absolute orientation: an orthonormal frame on the world side, one per root on the camera side
            const V3 w1 = divs(d12, sqrt(c2)), w3 = divs(cr, sqrt(cr2));
            const V3 w2 = cross(w3, w1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double v = y[k] - 0.25 * b;
                for (int it = 0; it < QUARTIC_POLISH; ++it) {
                    const double f = (((A4 * v + A3) * v + A2) * v + A1) * v + A0;
                    const double df = ((4.0 * A4 * v + 3.0 * A3) * v + 2.0 * A2) * v + A1;
                    if (df != 0.0) v = v - f / df;
                }
                const double Dv = e1 * v + e0;
                const double u = ((n2 * v + n1) * v + n0) / Dv;
                const double den = (1.0 + v * v) - (2.0 * v) * cb;
                const double s1 = sqrt(b2 / den), s2 = u * s1, s3 = v * s1;
                bool good = ok[k] && fin(v) && v > 0.0 && u > 0.0 && den > 0.0 && fin(s1) && fin(s2) && fin(s3) && s1 > 0.0;
                const V3 C1 = scale(j1, s1), C2 = scale(j2, s2), C3 = scale(j3, s3);
                const V3 g12 = sub(C2, C1), g13 = sub(C3, C1);
                const V3 f1 = divs(g12, sqrt(dot(g12, g12)));
                const V3 fc = cross(g12, g13);
                const V3 f3 = divs(fc, sqrt(dot(fc, fc)));
                const V3 f2 = cross(f3, f1);
                double R[12];
                R[0] = f1.x * w1.x + f2.x * w2.x + f3.x * w3.x; R[1] = f1.x * w1.y + f2.x * w2.y + f3.x * w3.y; R[2] = f1.x * w1.z + f2.x * w2.z + f3.x * w3.z;
                R[4] = f1.y * w1.x + f2.y * w2.x + f3.y * w3.x; R[5] = f1.y * w1.y + f2.y * w2.y + f3.y * w3.y; R[6] = f1.y * w1.z + f2.y * w2.z + f3.y * w3.z;
                R[8] = f1.z * w1.x + f2.z * w2.x + f3.z * w3.x; R[9] = f1.z * w1.y + f2.z * w2.y + f3.z * w3.y; R[10] = f1.z * w1.z + f2.z * w2.z + f3.z * w3.z;
                R[3] = C1.x - (R[0] * P1.x + R[1] * P1.y + R[2] * P1.z);
                R[7] = C1.y - (R[4] * P1.x + R[5] * P1.y + R[6] * P1.z);
                R[11] = C1.z - (R[8] * P1.x + R[9] * P1.y + R[10] * P1.z);
#pragma unroll
                for (int e_ = 0; e_ < 12; ++e_) good = good && fin(R[e_]);
                if (good) {      // compact the valid roots to the front, in slot order (ns <= k: static indices after unrolling)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        if (kk == ns)
#pragma unroll
                            for (int e_ = 0; e_ < 12; ++e_) sol[kk][e_] = R[e_];
                    ++ns;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 12; ++e) out[k * 12 + e] = sol[k][e];
    n_sol[slot] = ns;
    if (triples) { triples[slot * 3] = i0; triples[slot * 3 + 1] = i1; triples[slot * 3 + 2] = i2; }
}

// ---------------------------------------------------------------- score: (hypotheses x rows) reprojection tests
// One workgroup per (pair, SCORE_TRIALS trials): the pair's rows go through LDS in chunks of SCORE_CHUNK (structure of arrays: lanes
// read consecutive doubles), each wave takes SCORE_TPW trials in turn per chunk, the four root slots of a trial scored together from
// registers, lanes striding over the rows.  Slots beyond n_sol hold zeros: depth 0, no inlier.
__global__ __launch_bounds__(256) void pose_score_kernel(const double* __restrict__ pts, const double* __restrict__ xyz,
                                                         const int* __restrict__ count, const double* __restrict__ poses,
                                                         const int* __restrict__ n_sol, const int* __restrict__ cam_model,
                                                         const double* __restrict__ cam_params, int seg_k, int t0, int trials,
                                                         double threshold_px, int* __restrict__ h_inl, double* __restrict__ h_res) {
    __shared__ double rows[5][SCORE_CHUNK];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tr0 = blockIdx.x * SCORE_TRIALS + wave * SCORE_TPW;
    int n = count[p];
    n = n > t0 ? t0 : (n < 0 ? 0 : n);
    const int b = p / seg_k;
    const Cam cam = cam_unify(cam_model[b], cam_params + (size_t)b * PRAM_POSE_CAM_PARAMS);
    const double th = threshold_px / ((cam.fx + cam.fy) / 2.0);
    const double thr2 = th * th;
    int cnt[SCORE_TPW][4];
    double res[SCORE_TPW][4];
#pragma unroll
    for (int t = 0; t < SCORE_TPW; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) { cnt[t][k] = 0; res[t][k] = 0.0; }
    const double* pb = pts + (size_t)p * t0 * 2;
    const double* xb = xyz + (size_t)p * t0 * 3;
    for (int c0 = 0; c0 < n; c0 += SCORE_CHUNK) {
        const int len = n - c0 < SCORE_CHUNK ? n - c0 : SCORE_CHUNK;
        __syncthreads();
        for (int i = tid; i < len; i += 256) {
            const size_t r = (size_t)(c0 + i);
            rows[0][i] = pb[r * 2]; rows[1][i] = pb[r * 2 + 1];
            rows[2][i] = xb[r * 3]; rows[3][i] = xb[r * 3 + 1]; rows[4][i] = xb[r * 3 + 2];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < SCORE_TPW; ++t) {
            if (tr0 + t >= trials) continue;      // uniform over the wave
            const double* ps = poses + ((size_t)p * trials + tr0 + t) * 48;
            double P[4][12];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int e = 0; e < 12; ++e) P[k][e] = ps[k * 12 + e];
            for (int i = lane; i < len; i += 64) {
                const double px = rows[0][i], py = rows[1][i], X = rows[2][i], Y = rows[3][i], Z = rows[4][i];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double xc = P[k][0] * X + P[k][1] * Y + P[k][2] * Z + P[k][3];
                    const double yc = P[k][4] * X + P[k][5] * Y + P[k][6] * Z + P[k][7];
                    const double zc = P[k][8] * X + P[k][9] * Y + P[k][10] * Z + P[k][11];
                    const double du = xc / zc - px, dv = yc / zc - py;
                    const double e = du * du + dv * dv;
                    const bool in = zc > 0.0 && e <= thr2;
                    cnt[t][k] += in;
                    res[t][k] += in ? e : 0.0;
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < SCORE_TPW; ++t) {
        if (tr0 + t >= trials) continue;
        const size_t slot = (size_t)p * trials + tr0 + t;
        const int ns = n_sol[slot];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = wave_sum_i32(cnt[t][k]);
            const double s = wave_sum_f64(res[t][k]);
            if (lane == 0) {
                h_inl[slot * 4 + k] = k < ns ? c : -1;      // -1 = no hypothesis in this slot
                h_res[slot * 4 + k] = k < ns ? s : 0.0;
            }
        }
    }
}

// ---------------------------------------------------------------- refine: LM on the inliers, re-score, refine, final state
constexpr int LM_VALS = 28;      // cost, 21 of J^T W J (upper triangle, row-major), 6 of J^T W r

__device__ __forceinline__ bool row_inlier(const Pose& q, const double* __restrict__ pt, const double* __restrict__ X, double thr2) {
    const double xc = q.R[0] * X[0] + q.R[1] * X[1] + q.R[2] * X[2] + q.t[0];
    const double yc = q.R[3] * X[0] + q.R[4] * X[1] + q.R[5] * X[2] + q.t[1];
    const double zc = q.R[6] * X[0] + q.R[7] * X[1] + q.R[8] * X[2] + q.t[2];
    const double du = xc / zc - pt[0], dv = yc / zc - pt[1];
    return zc > 0.0 && du * du + dv * dv <= thr2;
}

// marks the inliers of q (one byte per row, thread tid owns rows tid, tid + 256, ...) and returns their number to every thread
__device__ int mark_inliers(const Pose& q, const double* __restrict__ pb, const double* __restrict__ xb, int n, double thr2,
                            unsigned char* __restrict__ mask, int* sred) {
    int c = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const bool in = row_inlier(q, pb + (size_t)i * 2, xb + (size_t)i * 3, thr2);
        mask[i] = in;
        c += in;
    }
    return block_sum_i32<4>(c, sred);
}

// cost, J^T W J, J^T W r over the masked rows at pose q -> tot[LM_VALS] in LDS (every thread may read it after the call)
__device__ void lm_pass(const Pose& q, const Cam& cam, const float* __restrict__ kb, const double* __restrict__ xb, int n,
                        const unsigned char* __restrict__ mask, double (*wred)[LM_VALS], double* tot) {
    double acc[LM_VALS];
#pragma unroll
    for (int e = 0; e < LM_VALS; ++e) acc[e] = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        if (!mask[i]) continue;
        const double* X = xb + (size_t)i * 3;
        const double Y0 = q.R[0] * X[0] + q.R[1] * X[1] + q.R[2] * X[2];
        const double Y1 = q.R[3] * X[0] + q.R[4] * X[1] + q.R[5] * X[2];
        const double Y2 = q.R[6] * X[0] + q.R[7] * X[1] + q.R[8] * X[2];
        const double xc = Y0 + q.t[0], yc = Y1 + q.t[1], z = Y2 + q.t[2];
        if (!(z > 1e-12)) continue;
        const double u = xc / z, v = yc / z;
        double ud, vd, j11, j12, j22;
        distort(cam, u, v, ud, vd);
        const double r0 = cam.fx * ud + cam.cx - ((double)kb[(size_t)i * 2] + 0.5);
        const double r1 = cam.fy * vd + cam.cy - ((double)kb[(size_t)i * 2 + 1] + 0.5);
        const double s = r0 * r0 + r1 * r1;
        if (!fin(s)) continue;
        distort_jac(cam, u, v, j11, j12, j22);
        const double iz = 1.0 / z;
        double J[2][6];
        const double a00 = cam.fx * j11 * iz, a01 = cam.fx * j12 * iz, a02 = -cam.fx * (j11 * u + j12 * v) * iz;
        const double a10 = cam.fy * j12 * iz, a11 = cam.fy * j22 * iz, a12 = -cam.fy * (j12 * u + j22 * v) * iz;
        J[0][0] = a02 * Y1 - a01 * Y2; J[0][1] = a00 * Y2 - a02 * Y0; J[0][2] = a01 * Y0 - a00 * Y1; J[0][3] = a00; J[0][4] = a01; J[0][5] = a02;
        J[1][0] = a12 * Y1 - a11 * Y2; J[1][1] = a10 * Y2 - a12 * Y0; J[1][2] = a11 * Y0 - a10 * Y1; J[1][3] = a10; J[1][4] = a11; J[1][5] = a12;
        const double w = 1.0 / (1.0 + s);      // Cauchy, scale 1 px: rho(s) = log(1 + s), rho' = 1 / (1 + s)
        acc[0] += log1p(s);
        int e = 1;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) acc[e++] += w * (J[0][a] * J[0][c] + J[1][a] * J[1][c]);
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[22 + a] += w * (J[0][a] * r0 + J[1][a] * r1);
    }
    block_fold_f64<LM_VALS>(acc, wred, tot);
}

struct LmShared {
    LmState<Pose, LM_VALS> lm;
    int sred[4];
};

__global__ __launch_bounds__(256) void pose_refine_kernel(const float* __restrict__ kpts, const double* __restrict__ pts,
                                                          const double* __restrict__ xyz, const int* __restrict__ count,
                                                          const double* __restrict__ poses, const int* __restrict__ h_inl,
                                                          const int* __restrict__ best, const int* __restrict__ cam_model,
                                                          const double* __restrict__ cam_params, int seg_k, int t0, int trials,
                                                          double threshold_px, double min_inlier_ratio, int iters,
                                                          double* __restrict__ qvec, double* __restrict__ tvec,
                                                          unsigned char* __restrict__ inliers, int* __restrict__ num_inliers,
                                                          int* __restrict__ success) {
    __shared__ LmShared sh;
    const int p = blockIdx.x, tid = threadIdx.x;
    int n = count[p];
    n = n > t0 ? t0 : (n < 0 ? 0 : n);
    unsigned char* mask = inliers + (size_t)p * t0;
    const int bi = best[p];
    const int n0 = bi >= 0 ? h_inl[(size_t)p * trials * 4 + bi] : 0;
    if (n < 3 || bi < 0 || n0 < 3 || (double)n0 < min_inlier_ratio * (double)n) {      // uniform: the reference's failed result
        for (int i = tid; i < t0; i += 256) mask[i] = 0;
        if (tid < 4) qvec[(size_t)p * 4 + tid] = 0.0;
        if (tid < 3) tvec[(size_t)p * 3 + tid] = 0.0;
        if (tid == 0) { num_inliers[p] = 0; success[p] = 0; }
        return;
    }
    const int b = p / seg_k;
    const Cam cam = cam_unify(cam_model[b], cam_params + (size_t)b * PRAM_POSE_CAM_PARAMS);
    const double th = threshold_px / ((cam.fx + cam.fy) / 2.0);
    const double thr2 = th * th;
    const float* kb = kpts + (size_t)p * t0 * 2;
    const double* pb = pts + (size_t)p * t0 * 2;
    const double* xb = xyz + (size_t)p * t0 * 3;
    const double* hp = poses + ((size_t)p * trials * 4 + bi) * 12;
    Pose h;
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 3; ++c) h.R[a * 3 + c] = hp[a * 4 + c];
        h.t[a] = hp[a * 4 + 3];
    }
    Pose q = h;
    // `iters` Levenberg-Marquardt iterations from q on the masked rows; every thread ends with the same pose
    const auto pass = [&](const Pose& m) { lm_pass(m, cam, kb, xb, n, mask, sh.lm.wred, sh.lm.tot); };
    const auto step = [](const double* cur, double lam, const Pose& from, Pose& cand) {
        double d[6];
        const bool okd = chol_solve6(cur + 1, cur + 22, lam, d);
        if (okd) pose_update(from, d, cand);
        return okd;
    };
    mark_inliers(q, pb, xb, n, thr2, mask, sh.sred);
    lm_refine(q, iters, sh.lm, pass, step);
    mark_inliers(q, pb, xb, n, thr2, mask, sh.sred);
    lm_refine(q, iters, sh.lm, pass, step);
    int n2 = mark_inliers(q, pb, xb, n, thr2, mask, sh.sred);
    if (n2 < n0 || !pose_finite(q)) {      // the refined pose lost support: the hypothesis stands
        q = h;
        n2 = mark_inliers(q, pb, xb, n, thr2, mask, sh.sred);
    }
    for (int i = n + tid; i < t0; i += 256) mask[i] = 0;
    if (tid == 0) {
        double qv[4];
        rot_to_qvec(q.R, qv);
        for (int a = 0; a < 4; ++a) qvec[(size_t)p * 4 + a] = qv[a];
        for (int a = 0; a < 3; ++a) tvec[(size_t)p * 3 + a] = q.t[a];
        num_inliers[p] = n2;
        success[p] = 1;
    }
}

// ---------------------------------------------------------------- select: the candidate loop's verify_and_update, after the fact
__global__ __launch_bounds__(64) void pose_select_kernel(const int* __restrict__ success, const int* __restrict__ num_inliers, int batch,
                                                         int seg_k, int min_inliers, int* __restrict__ chosen) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    int kept = -1, status = -1;
    for (int w = 0; w < seg_k; ++w) {
        const int p = b * seg_k + w;
        if (!success[p]) continue;
        if (kept < 0 || num_inliers[b * seg_k + kept] < num_inliers[p]) kept = w;      // multimap3d.py:297
        if (num_inliers[p] < min_inliers) { status = 0; continue; }
        status = 1;
        break;
    }
    // the reference sets ret['order'] = i, the position in the vote: the order of the kept candidate IS its index
    chosen[b * 3] = kept; chosen[b * 3 + 1] = status; chosen[b * 3 + 2] = kept;
}

}  // namespace

extern "C" int pram_pose_prepare(const float* m_kpts, const int* count, const int* cam_model, const double* cam_params,
                                 const int* cam_model_host, int batch, int seg_k, int t0, double* norm_pts, void* stream) {
    PRAM_REQUIRE(m_kpts && count && cam_model && cam_params && cam_model_host && norm_pts, "pram_pose_prepare: null pointer");
    PRAM_REQUIRE(aligned(m_kpts, 4) && aligned(count, 4) && aligned(cam_model, 4) && aligned(cam_params, 8) && aligned(norm_pts, 8),
                 "pram_pose_prepare: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && seg_k >= 1 && t0 >= 0 && (long long)batch * seg_k <= 65535, "pram_pose_prepare: needs batch >= 0, seg_k >= 1, t0 >= 0, batch * seg_k <= 65535");
    for (int b = 0; b < batch; ++b)
        if (cam_model_host[b] < PRAM_CAM_SIMPLE_PINHOLE || cam_model_host[b] > PRAM_CAM_OPENCV) {
            pram_set_error("pram_pose_prepare: camera model id %d of query %d is not supported", cam_model_host[b], b);
            return PRAM_E_UNSUPPORTED;
        }
    if (batch == 0 || t0 == 0) return PRAM_OK;
    hipLaunchKernelGGL(pose_prepare_kernel, dim3(cdiv(t0, 256), batch * seg_k), dim3(256), 0, (hipStream_t)stream, m_kpts, count, cam_model,
                       cam_params, seg_k, t0, norm_pts);
    return pram_launch_status("pram_pose_prepare");
}

extern "C" int pram_pose_hypotheses(const double* norm_pts, const double* m_xyz, const int* count, int pairs, int t0, int trials,
                                    unsigned long long seed, double* poses, int* n_sol, int* triples, void* stream) {
    PRAM_REQUIRE(norm_pts && m_xyz && count && poses && n_sol, "pram_pose_hypotheses: null pointer");
    PRAM_REQUIRE(aligned(norm_pts, 8) && aligned(m_xyz, 8) && aligned(count, 4) && aligned(poses, 8) && aligned(n_sol, 4) && aligned(triples, 4),
                 "pram_pose_hypotheses: misaligned pointer");
    PRAM_REQUIRE(pairs >= 0 && pairs <= 65535 && t0 >= 0 && trials >= 1 && trials <= (1 << 24), "pram_pose_hypotheses: needs 0 <= pairs <= 65535, t0 >= 0, 1 <= trials <= 2^24");
    if (pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(pose_hypotheses_kernel, dim3(cdiv(trials, 256), pairs), dim3(256), 0, (hipStream_t)stream, norm_pts, m_xyz, count, t0,
                       trials, seed, poses, n_sol, triples);
    return pram_launch_status("pram_pose_hypotheses");
}

extern "C" int pram_pose_score(const double* norm_pts, const double* m_xyz, const int* count, const double* poses, const int* n_sol,
                               const int* cam_model, const double* cam_params, int pairs, int seg_k, int t0, int trials,
                               double threshold_px, int* h_inliers, double* h_resid, int* best, void* stream) {
    PRAM_REQUIRE(norm_pts && m_xyz && count && poses && n_sol && cam_model && cam_params && h_inliers && h_resid && best, "pram_pose_score: null pointer");
    PRAM_REQUIRE(aligned(norm_pts, 8) && aligned(m_xyz, 8) && aligned(count, 4) && aligned(poses, 8) && aligned(n_sol, 4) && aligned(cam_model, 4) &&
                 aligned(cam_params, 8) && aligned(h_inliers, 4) && aligned(h_resid, 8) && aligned(best, 4), "pram_pose_score: misaligned pointer");
    PRAM_REQUIRE(pairs >= 0 && pairs <= 65535 && seg_k >= 1 && pairs % seg_k == 0 && t0 >= 0 && trials >= 1 && trials <= (1 << 24) && threshold_px > 0.0,
                 "pram_pose_score: needs 0 <= pairs <= 65535 (a multiple of seg_k >= 1), t0 >= 0, 1 <= trials <= 2^24, threshold_px > 0");
    if (pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(pose_score_kernel, dim3(cdiv(trials, SCORE_TRIALS), pairs), dim3(256), 0, (hipStream_t)stream, norm_pts, m_xyz, count, poses,
                       n_sol, cam_model, cam_params, seg_k, t0, trials, threshold_px, h_inliers, h_resid);
    hipLaunchKernelGGL(ransac_pick_kernel, dim3(pairs), dim3(256), 0, (hipStream_t)stream, h_inliers, h_resid, trials * 4, best);
    return pram_launch_status("pram_pose_score");
}

extern "C" int pram_pose_refine(const float* m_kpts, const double* norm_pts, const double* m_xyz, const int* count, const double* poses,
                                const int* h_inliers, const int* best, const int* cam_model, const double* cam_params, int pairs, int seg_k,
                                int t0, int trials, double threshold_px, double min_inlier_ratio, int refine_iters, double* qvec, double* tvec,
                                unsigned char* inliers, int* num_inliers, int* success, void* stream) {
    PRAM_REQUIRE(m_kpts && norm_pts && m_xyz && count && poses && h_inliers && best && cam_model && cam_params && qvec && tvec && inliers &&
                 num_inliers && success, "pram_pose_refine: null pointer");
    PRAM_REQUIRE(aligned(m_kpts, 4) && aligned(norm_pts, 8) && aligned(m_xyz, 8) && aligned(count, 4) && aligned(poses, 8) && aligned(h_inliers, 4) &&
                 aligned(best, 4) && aligned(cam_model, 4) && aligned(cam_params, 8) && aligned(qvec, 8) && aligned(tvec, 8) && aligned(num_inliers, 4) &&
                 aligned(success, 4), "pram_pose_refine: misaligned pointer");
    PRAM_REQUIRE(pairs >= 0 && seg_k >= 1 && pairs % seg_k == 0 && t0 >= 0 && trials >= 1 && trials <= (1 << 24) && threshold_px > 0.0 &&
                 min_inlier_ratio >= 0.0 && refine_iters >= 0 && refine_iters <= 1000,
                 "pram_pose_refine: needs pairs >= 0 (a multiple of seg_k >= 1), t0 >= 0, 1 <= trials <= 2^24, threshold_px > 0, min_inlier_ratio >= 0, 0 <= refine_iters <= 1000");
    if (pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(pose_refine_kernel, dim3(pairs), dim3(256), 0, (hipStream_t)stream, m_kpts, norm_pts, m_xyz, count, poses, h_inliers, best,
                       cam_model, cam_params, seg_k, t0, trials, threshold_px, min_inlier_ratio, refine_iters, qvec, tvec, inliers, num_inliers,
                       success);
    return pram_launch_status("pram_pose_refine");
}

extern "C" int pram_pose_select(const int* success, const int* num_inliers, int batch, int seg_k, int min_inliers, int* chosen, void* stream) {
    PRAM_REQUIRE(success && num_inliers && chosen, "pram_pose_select: null pointer");
    PRAM_REQUIRE(aligned(success, 4) && aligned(num_inliers, 4) && aligned(chosen, 4), "pram_pose_select: misaligned pointer");
    PRAM_REQUIRE(batch >= 0 && seg_k >= 1, "pram_pose_select: needs batch >= 0, seg_k >= 1");
    if (batch == 0) return PRAM_OK;
    hipLaunchKernelGGL(pose_select_kernel, dim3(cdiv(batch, 64)), dim3(64), 0, (hipStream_t)stream, success, num_inliers, batch, seg_k, min_inliers,
                       chosen);
    return pram_launch_status("pram_pose_select");
}
