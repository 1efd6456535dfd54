// What the float64 geometry kernels share (pose.hip, twoview.hip, triangulate.hip, and through obs.h and ransac.h bundle.hip and
// mapper.hip): COLMAP's camera models unified to OPENCV, its distortion function and Jacobian, the 3-vector helpers and the
// counter-based sampler's mixing function.  The sums of a wave and of a workgroup are workgroup.h's, included from here.
#pragma once
#include "workgroup.h"
#include <math.h>

struct Cam { double fx, fy, cx, cy, k1, k2, p1, p2; };

// every supported model is OPENCV with some coefficients zero (COLMAP's parameter order)
__device__ __forceinline__ Cam cam_unify(int model, const double* __restrict__ p) {
    Cam c;
    switch (model) {
        case PRAM_CAM_PINHOLE: c = {p[0], p[1], p[2], p[3], 0.0, 0.0, 0.0, 0.0}; break;
        case PRAM_CAM_SIMPLE_RADIAL: c = {p[0], p[0], p[1], p[2], p[3], 0.0, 0.0, 0.0}; break;
        case PRAM_CAM_RADIAL: c = {p[0], p[0], p[1], p[2], p[3], p[4], 0.0, 0.0}; break;
        case PRAM_CAM_OPENCV: c = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]}; break;
        default: c = {p[0], p[0], p[1], p[2], 0.0, 0.0, 0.0, 0.0}; break;      // PRAM_CAM_SIMPLE_PINHOLE
    }
    return c;
}

__device__ __forceinline__ void distort(const Cam& c, double u, double v, double& ud, double& vd) {
    const double r2 = u * u + v * v;
    const double rad = c.k1 * r2 + c.k2 * r2 * r2;
    const double du = u * rad + 2.0 * c.p1 * u * v + c.p2 * (r2 + 2.0 * u * u);
    const double dv = v * rad + 2.0 * c.p2 * u * v + c.p1 * (r2 + 2.0 * v * v);
    ud = u + du; vd = v + dv;
}

__device__ __forceinline__ void distort_jac(const Cam& c, double u, double v, double& j11, double& j12, double& j22) {
    const double r2 = u * u + v * v;
    const double rad = c.k1 * r2 + c.k2 * r2 * r2;
    const double dr = c.k1 + 2.0 * c.k2 * r2;
    j11 = 1.0 + rad + 2.0 * u * u * dr + 2.0 * c.p1 * v + 6.0 * c.p2 * u;
    j12 = 2.0 * u * v * dr + 2.0 * c.p1 * u + 2.0 * c.p2 * v;
    j22 = 1.0 + rad + 2.0 * v * v * dr + 2.0 * c.p2 * u + 6.0 * c.p1 * v;
}

// the number of parameters of a model (COLMAP's), and how many of the first are focal lengths
__device__ __forceinline__ int cam_n_params(int model) {
    switch (model) {
        case PRAM_CAM_PINHOLE: case PRAM_CAM_SIMPLE_RADIAL: return 4;
        case PRAM_CAM_RADIAL: return 5;
        case PRAM_CAM_OPENCV: return 8;
        default: return 3;
    }
}
__device__ __forceinline__ int cam_n_focal(int model) { return model == PRAM_CAM_PINHOLE || model == PRAM_CAM_OPENCV ? 2 : 1; }

// d residual / d (the model's own parameters, COLMAP's order): J [2][8], zero padded.  u, v: the normalised point; ud, vd: the
// distorted point; r2 = u^2 + v^2 (obs_residual's).  A model with one focal length has the column (ud, vd) for f.
__device__ __forceinline__ void cam_param_jac(int model, const Cam& c, double u, double v, double ud, double vd, double r2, double* J) {
#pragma unroll
    for (int e = 0; e < 16; ++e) J[e] = 0.0;
    const double k1u = c.fx * u * r2, k1v = c.fy * v * r2, k2u = c.fx * u * r2 * r2, k2v = c.fy * v * r2 * r2;
    switch (model) {
        case PRAM_CAM_PINHOLE: J[0] = ud; J[9] = vd; J[2] = 1.0; J[11] = 1.0; break;
        case PRAM_CAM_SIMPLE_RADIAL: J[0] = ud; J[8] = vd; J[1] = 1.0; J[10] = 1.0; J[3] = k1u; J[11] = k1v; break;
        case PRAM_CAM_RADIAL: J[0] = ud; J[8] = vd; J[1] = 1.0; J[10] = 1.0; J[3] = k1u; J[11] = k1v; J[4] = k2u; J[12] = k2v; break;
        case PRAM_CAM_OPENCV:
            J[0] = ud; J[9] = vd; J[2] = 1.0; J[11] = 1.0; J[4] = k1u; J[12] = k1v; J[5] = k2u; J[13] = k2v;
            J[6] = c.fx * (2.0 * u * v); J[14] = c.fy * (r2 + 2.0 * v * v);
            J[7] = c.fx * (r2 + 2.0 * u * u); J[15] = c.fy * (2.0 * u * v);
            break;
        default: J[0] = ud; J[8] = vd; J[1] = 1.0; J[10] = 1.0; break;      // PRAM_CAM_SIMPLE_PINHOLE
    }
}

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double angle(V3 a, V3 b) { const V3 c = cross(a, b); return atan2(sqrt(dot(c, c)), dot(a, b)); }
__device__ __forceinline__ bool fin(double x) { return isfinite(x); }

__device__ __forceinline__ unsigned long long sm64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
