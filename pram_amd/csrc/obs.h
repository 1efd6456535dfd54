// The observation model the map kernels share (triangulate.hip, bundle.hip, mapper.hip): keypoint (row) r seen in frame f of the
// frame table, its ray, residual and midpoint, and the 3 x 3 Cholesky solve of a point's normal equations.  camera.h brings the
// camera model and, through workgroup.h, the sums.
#pragma once
#include "camera.h"

constexpr int FC = PRAM_TRI_FRAME_COLS;      // R [9] row-major, t [3], C = -R^T t [3], mean focal length

// What stage 2b and stage 4 compute of an observation, once, so that the two agree to the bit.  A caller passes a row and a
// frame the tables hold.
struct Obs {
    const double* norm; const float* kpts; const double* table; const int* cam_model; const double* cam_params; int n_frames, n_rows;
};

__device__ __forceinline__ V3 obs_centre(const Obs& g, int f) {
    const double* T = g.table + (size_t)f * FC;
    return {T[12], T[13], T[14]};
}

// the observation's unit ray in world coordinates: R^T (u, v, 1) / |(u, v, 1)|
__device__ __forceinline__ V3 obs_ray(const Obs& g, int r, int f) {
    const double* T = g.table + (size_t)f * FC;
    const double u = g.norm[(size_t)r * 2], v = g.norm[(size_t)r * 2 + 1];
    const double n = sqrt(u * u + v * v + 1.0);
    const double x = u / n, y = v / n, z = 1.0 / n;
    return {T[0] * x + T[3] * y + T[6] * z, T[1] * x + T[4] * y + T[7] * z, T[2] * x + T[5] * y + T[8] * z};
}

__device__ __forceinline__ double obs_depth(const Obs& g, int f, V3 X) {
    const double* T = g.table + (size_t)f * FC;
    return T[6] * X.x + T[7] * X.y + T[8] * X.z + T[11];
}

// pixel residual of X through the full camera model, against keypoint + 0.5; z: the depth; with_jac: J [2][3] = d residual / d X
__device__ __forceinline__ void obs_residual(const Obs& g, int row, int f, V3 X, double& z, double& r0, double& r1, bool with_jac, double* J) {
    const double* T = g.table + (size_t)f * FC;
    const Cam c = cam_unify(g.cam_model[f], g.cam_params + (size_t)f * PRAM_POSE_CAM_PARAMS);
    const size_t r = (size_t)row;
    const double xc = T[0] * X.x + T[1] * X.y + T[2] * X.z + T[9];
    const double yc = T[3] * X.x + T[4] * X.y + T[5] * X.z + T[10];
    z = T[6] * X.x + T[7] * X.y + T[8] * X.z + T[11];
    const double u = xc / z, v = yc / z;
    double ud, vd;
    distort(c, u, v, ud, vd);
    r0 = c.fx * ud + c.cx - ((double)g.kpts[r * 2] + 0.5);
    r1 = c.fy * vd + c.cy - ((double)g.kpts[r * 2 + 1] + 0.5);
    if (with_jac) {
        double j11, j12, j22;
        distort_jac(c, u, v, j11, j12, j22);
        const double iz = 1.0 / z;
        const double a00 = c.fx * j11 * iz, a01 = c.fx * j12 * iz, a02 = -c.fx * (j11 * u + j12 * v) * iz;
        const double a10 = c.fy * j12 * iz, a11 = c.fy * j22 * iz, a12 = -c.fy * (j12 * u + j22 * v) * iz;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            J[k] = a00 * T[k] + a01 * T[3 + k] + a02 * T[6 + k];
            J[3 + k] = a10 * T[k] + a11 * T[3 + k] + a12 * T[6 + k];
        }
    }
}

// squared reprojection error and the inlier test: positive depth and error <= thr (NaN compares false)
__device__ __forceinline__ bool obs_inlier(const Obs& g, int r, int f, V3 X, double thr2, double& err2) {
    double z, r0, r1;
    obs_residual(g, r, f, X, z, r0, r1, false, nullptr);
    err2 = r0 * r0 + r1 * r1;
    return z > 0.0 && err2 <= thr2;
}

// the midpoint of the closest points of two rays: stage 4's hypothesis, stage 2b's point, the mapper's seed score
__device__ __forceinline__ V3 ray_midpoint(V3 C1, V3 d1, V3 C2, V3 d2) {
    const V3 w = sub(C1, C2);
    const double a = dot(d1, d1), b = dot(d1, d2), c = dot(d2, d2), d = dot(d1, w), e = dot(d2, w);
    const double den = a * c - b * b;
    const double s = (b * e - c * d) / den, u = (a * e - b * d) / den;
    return {0.5 * ((C1.x + s * d1.x) + (C2.x + u * d2.x)), 0.5 * ((C1.y + s * d1.y) + (C2.y + u * d2.y)),
            0.5 * ((C1.z + s * d1.z) + (C2.z + u * d2.z))};
}

// A x = b for a symmetric A given as a00 a01 a02 a11 a12 a22, by Cholesky; false when a pivot is not positive or x is not finite
static __device__ bool chol_solve3(const double* __restrict__ A, const double* __restrict__ b, double* x) {
    if (!(A[0] > 0.0)) return false;
    const double l00 = sqrt(A[0]), l10 = A[1] / l00, l20 = A[2] / l00;
    const double d1 = A[3] - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1), l21 = (A[4] - l20 * l10) / l11;
    const double d2 = A[5] - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    const double y0 = b[0] / l00, y1 = (b[1] - l10 * y0) / l11, y2 = (b[2] - l20 * y0 - l21 * y1) / l22;
    x[2] = y2 / l22;
    x[1] = (y1 - l21 * x[2]) / l11;
    x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
    return fin(x[0]) && fin(x[1]) && fin(x[2]);
}
