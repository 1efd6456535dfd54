// Two-view geometry without poses (what estimation_and_geometric_verification of the reference's localization/triangulation.py asks of
// pycolmap.verify_matches): per pair of frames an essential matrix by RANSAC over five-point samples with a fixed trial budget, the
// mask of the matches that agree with it, its decomposition into a relative pose and a 5-DoF Levenberg-Marquardt refinement, in
// pram_tri_verify's output layout.  float64 throughout; every loop has a compile-time or argument-given bound.  DESIGN.md 4.24 has the
// layout, the formulas and the deviations from COLMAP's estimator.
#include "camera.h"
#include "glue.h"
#include "launch.h"
#include "ransac.h"
#include <math.h>

namespace {

constexpr int MAX_SOL = PRAM_TWOVIEW_MAX_SOL;
constexpr int BISECT = 48;                // bisection steps per root on the Sturm count
constexpr int NEWTON = 4;                 // Newton steps per root on det B(z)
constexpr double CHECK_TOL = 1e-6;        // a root is kept when det E and 2 E E^T E - tr(E E^T) E stay below it (|E|_F = 1)
constexpr double RANK_EPS = 1e-10;        // a pivot of the 5 x 9 system below RANK_EPS * the first pivot: rank-deficient
constexpr int SCORE_CHUNK = 768;          // rows per LDS chunk: 4 doubles each = 24 KB (always chunked, whatever the count)
constexpr int SCORE_TPW = 2;              // trials a wave takes in turn on every chunk
constexpr int SCORE_TRIALS = 4 * SCORE_TPW;      // trials per workgroup
constexpr int SCORE_HALF = MAX_SOL / 2;   // solution slots scored together from registers
constexpr int LM_VALS = 21;               // cost, 15 of J^T W J (upper triangle, row-major), 5 of J^T W r

// ---------------------------------------------------------------- a pair's rows: (u0, v0, u1, v1) of a match, NaN outside a frame
struct PairRows {
    const double* norm; const int* matches;
    int r0, n0, r1, n1, m0, n;      // first row and length of the two frames, first match and their number
    bool ok;
};

__device__ __forceinline__ PairRows pair_rows(const double* __restrict__ norm, const int* __restrict__ frame_off, const int* __restrict__ pairs,
                                              const int* __restrict__ m_off, const int* __restrict__ matches, int n_frames, int n_matches, int p) {
    PairRows g = {norm, matches, 0, 0, 0, 0, 0, 0, false};
    const int f0 = pairs[(size_t)p * 2], f1 = pairs[(size_t)p * 2 + 1];
    int m1;
    clamped_range(m_off[p], m_off[p + 1], n_matches, g.m0, m1);
    g.n = m1 - g.m0;
    g.ok = f0 >= 0 && f0 < n_frames && f1 >= 0 && f1 < n_frames;
    if (g.ok) {
        g.r0 = frame_off[f0]; g.n0 = frame_off[f0 + 1] - g.r0;
        g.r1 = frame_off[f1]; g.n1 = frame_off[f1 + 1] - g.r1;
    }
    return g;
}

// match i of the pair (0 <= i < g.n); false, and NaN, when an index is outside its frame: nothing is dereferenced then
__device__ __forceinline__ bool load_row(const PairRows& g, int i, double& u0, double& v0, double& u1, double& v1) {
    const int i0 = g.matches[(size_t)(g.m0 + i) * 2], i1 = g.matches[(size_t)(g.m0 + i) * 2 + 1];
    const bool in = g.ok && i0 >= 0 && i0 < g.n0 && i1 >= 0 && i1 < g.n1;
    u0 = v0 = u1 = v1 = NAN;
    if (in) {
        u0 = g.norm[(size_t)(g.r0 + i0) * 2]; v0 = g.norm[(size_t)(g.r0 + i0) * 2 + 1];
        u1 = g.norm[(size_t)(g.r1 + i1) * 2]; v1 = g.norm[(size_t)(g.r1 + i1) * 2 + 1];
    }
    return in;
}

// what a pixel is on the normalised plane of the pair: the mean of the two cameras' 1 / (mean focal length)
__device__ __forceinline__ double pixel_unit(const int* __restrict__ cam_model, const double* __restrict__ cam_params, int f0, int f1) {
    const Cam a = cam_unify(cam_model[f0], cam_params + (size_t)f0 * PRAM_POSE_CAM_PARAMS);
    const Cam b = cam_unify(cam_model[f1], cam_params + (size_t)f1 * PRAM_POSE_CAM_PARAMS);
    return 0.5 * (1.0 / ((a.fx + a.fy) / 2.0) + 1.0 / ((b.fx + b.fy) / 2.0));
}

// squared Sampson error of x1^T E x0 = 0 on the normalised plane (0 / 0 = NaN for an empty slot: never an inlier)
__device__ __forceinline__ double sampson(const double* __restrict__ E, double u0, double v0, double u1, double v1) {
    const double a0 = (E[0] * u0 + E[1] * v0) + E[2], a1 = (E[3] * u0 + E[4] * v0) + E[5], a2 = (E[6] * u0 + E[7] * v0) + E[8];
    const double b0 = (E[0] * u1 + E[3] * v1) + E[6], b1 = (E[1] * u1 + E[4] * v1) + E[7];
    const double c = (u1 * a0 + v1 * a1) + a2;
    const double den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    return (c * c) / den;
}

// ---------------------------------------------------------------- hypotheses: sampler + five-point solver, one trial per lane
// The working set of a trial lives in LDS, element-major ([element][lane]: a wave's access to one element is 64 consecutive doubles,
// no bank conflict), so that every index below may be computed at run time without a private array going to scratch:
//   BAS  [4][9]    the null-space basis X, Y, Z, W of the 5 x 9 epipolar system
//   MAT  [10][20]  the constraint matrix; before it the 5 x 9 system; after the elimination B(z) [3][13] in its first rows and the
//                  Sturm chain [11][11] behind
//   TMP  [40]      degree-2 polynomials while the constraints are built; the column permutation; the products of det B(z)
constexpr int HYP_LANES = 64;
constexpr int BAS = 0, MAT = 36, TMP = 236, HYP_DOUBLES = 276;
constexpr int BZ = MAT, CHAIN = MAT + 40;
constexpr size_t HYP_LDS = (size_t)HYP_DOUBLES * HYP_LANES * sizeof(double);
#define LD(i) sh[(i) * HYP_LANES]

// monomials: degree 1 (x, y, z, 1); degree 2 (x2, xy, xz, y2, yz, z2, x, y, z, 1); degree 3 in Nister's column order (x3, y3, x2y, xy2,
// x2z, x2, y2z, y2, xyz, xy | xz2, xz, x, yz2, yz, y, z3, z2, z, 1).  T11 / T21: the product's index (tests/twoview_ref.py derives them).
__constant__ int T11[4][4] = {{0, 1, 2, 6}, {1, 3, 4, 7}, {2, 4, 5, 8}, {6, 7, 8, 9}};
__constant__ int T21[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {3, 1, 6, 7}, {8, 6, 13, 14}, {10, 13, 16, 17}, {5, 9, 11, 12},
                               {9, 7, 14, 15}, {11, 14, 17, 18}, {12, 15, 18, 19}};

// dst [10] += entry a x entry b of E as polynomials of degree 1 (entry e: BAS[m][e], m = x, y, z, 1)
__device__ __forceinline__ void acc11(double* sh, int dst, int a, int b) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) LD(dst + T11[i][j]) += LD(BAS + i * 9 + a) * LD(BAS + j * 9 + b);
}

// dst [20] += sign * (src [10] x entry b)
__device__ __forceinline__ void acc21(double* sh, int dst, int src, int b, double sign) {
    for (int i = 0; i < 10; ++i)
        for (int j = 0; j < 4; ++j) LD(dst + T21[i][j]) += sign * (LD(src + i) * LD(BAS + j * 9 + b));
}

__device__ __forceinline__ void zero(double* sh, int dst, int n) {
    for (int i = 0; i < n; ++i) LD(dst + i) = 0.0;
}

// dst [na + nb - 1] += sign * (a [na] * b [nb]), ascending coefficients
__device__ __forceinline__ void acc_conv(double* sh, int dst, int a, int na, int b, int nb, double sign) {
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) LD(dst + i + j) += sign * (LD(a + i) * LD(b + j));
}

__device__ __forceinline__ double horner(const double* sh, int c, int deg, double x) {
    double v = LD(c + deg);
    for (int i = deg - 1; i >= 0; --i) v = v * x + LD(c + i);
    return v;
}

// the sign changes of the Sturm chain at x (zeros are skipped)
__device__ __forceinline__ int sign_changes(const double* sh, double x) {
    int cnt = 0, last = 0;
    for (int i = 0; i < 11; ++i) {
        const double v = horner(sh, CHAIN + i * 11, 10 - i, x);
        const int sg = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
        cnt += sg != 0 && last != 0 && sg != last;
        last = sg != 0 ? sg : last;
    }
    return cnt;
}

// row k of B(z) and of B'(z): (p, q, r)(z)
__device__ __forceinline__ void bz_row(const double* sh, int k, double z, V3& val, V3& der) {
    double v[3], d[3];
    const int lo[3] = {0, 4, 8}, dg[3] = {3, 3, 4};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int c = BZ + k * 13 + lo[e];
        v[e] = horner(sh, c, dg[e], z);
        double dv = (double)dg[e] * LD(c + dg[e]);
        for (int i = dg[e] - 1; i > 0; --i) dv = dv * z + (double)i * LD(c + i);
        d[e] = dv;
    }
    val = {v[0], v[1], v[2]};
    der = {d[0], d[1], d[2]};
}

__device__ __forceinline__ double det3(V3 a, V3 b, V3 c) {
    return (a.x * (b.y * c.z - b.z * c.y) - a.y * (b.x * c.z - b.z * c.x)) + a.z * (b.x * c.y - b.y * c.x);
}

// the largest magnitude among det E and the entries of 2 E E^T E - tr(E E^T) E; infinity when it is not a number
__device__ __forceinline__ double violation(const double* e) {
    double worst = fabs((e[0] * (e[4] * e[8] - e[5] * e[7]) - e[1] * (e[3] * e[8] - e[5] * e[6])) + e[2] * (e[3] * e[7] - e[4] * e[6]));
    double G[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) G[i][j] = (e[3 * i] * e[3 * j] + e[3 * i + 1] * e[3 * j + 1]) + e[3 * i + 2] * e[3 * j + 2];
    const double tr = (G[0][0] + G[1][1]) + G[2][2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double c = 2.0 * ((G[i][0] * e[j] + G[i][1] * e[3 + j]) + G[i][2] * e[6 + j]) - tr * e[3 * i + j];
            worst = fmax(worst, fabs(c));      // fmax drops a NaN: caught below
            if (c != c) worst = INFINITY;
        }
    return worst == worst ? worst : INFINITY;
}

__global__ __launch_bounds__(HYP_LANES) void twoview_hypotheses_kernel(const double* __restrict__ norm, const int* __restrict__ frame_off,
                                                                       const int* __restrict__ pairs, const int* __restrict__ m_off,
                                                                       const int* __restrict__ matches, int n_frames, int n_matches, int pair0,
                                                                       int trials, unsigned long long seed, double* __restrict__ Es,
                                                                       int* __restrict__ n_sol, int* __restrict__ fives) {
    extern __shared__ __attribute__((aligned(16))) double hyp_lds[];
    const int p = blockIdx.y, lane = threadIdx.x, tr = blockIdx.x * HYP_LANES + lane;
    double* sh = hyp_lds + lane;
    const bool live = tr < trials;      // a lane beyond the budget computes on zeros and writes nothing
    const PairRows g = pair_rows(norm, frame_off, pairs, m_off, matches, n_frames, n_matches, p);
    const int n = g.n;
    // ---- the sampler: pick k from [0, n - k), stepped over the earlier picks in ascending order
    int pick[5] = {-1, -1, -1, -1, -1};
    bool ok = live && n >= 5;
    if (ok) {
        const unsigned long long key = sm64(sm64(seed) ^ (((unsigned long long)(unsigned)(pair0 + p) << 32) | (unsigned long long)(unsigned)tr));
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0;      // the earlier picks, ascending
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            int i = (int)__umul64hi(sm64(key + (unsigned long long)k), (unsigned long long)(n - k));
            if (k > 0) i += i >= s0;
            if (k > 1) i += i >= s1;
            if (k > 2) i += i >= s2;
            if (k > 3) i += i >= s3;
            pick[k] = i;
            // insert i into (s0 .. s_{k-1})
            if (k == 0) s0 = i;
            if (k == 1) { s1 = i > s0 ? i : s0; s0 = i > s0 ? s0 : i; }
            if (k == 2) { s2 = i; if (s2 < s1) { const int t = s1; s1 = s2; s2 = t; } if (s1 < s0) { const int t = s0; s0 = s1; s1 = t; } }
            if (k == 3) { s3 = i; if (s3 < s2) { const int t = s2; s2 = s3; s3 = t; } if (s2 < s1) { const int t = s1; s1 = s2; s2 = t; }
                          if (s1 < s0) { const int t = s0; s0 = s1; s1 = t; } }
        }
    }
    // ---- the 5 x 9 epipolar system in MAT: row s = x1 (x) x0, E row-major
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        double u0 = 0.0, v0 = 0.0, u1 = 0.0, v1 = 0.0;
        if (ok && !load_row(g, pick[s], u0, v0, u1, v1)) ok = false;
        if (!ok) u0 = v0 = u1 = v1 = 0.0;
        const double h0[3] = {u0, v0, 1.0}, h1[3] = {u1, v1, 1.0};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) LD(MAT + s * 9 + a * 3 + c) = ok ? h1[a] * h0[c] : 0.0;
    }
    // ---- its null space: Gauss-Jordan with complete pivoting, the column permutation in TMP
    for (int c = 0; c < 9; ++c) LD(TMP + c) = (double)c;
    double first = 0.0;
    for (int k = 0; k < 5; ++k) {
        double best = -1.0;
        int br = k, bc = k;
        for (int r = k; r < 5; ++r)
            for (int c = k; c < 9; ++c) {
                const double a = fabs(LD(MAT + r * 9 + c));
                if (a > best) { best = a; br = r; bc = c; }
            }
        if (k == 0) first = best;
        ok = ok && best > RANK_EPS * first;
        for (int c = 0; c < 9; ++c) { const double t = LD(MAT + k * 9 + c); LD(MAT + k * 9 + c) = LD(MAT + br * 9 + c); LD(MAT + br * 9 + c) = t; }
        for (int r = 0; r < 5; ++r) { const double t = LD(MAT + r * 9 + k); LD(MAT + r * 9 + k) = LD(MAT + r * 9 + bc); LD(MAT + r * 9 + bc) = t; }
        { const double t = LD(TMP + k); LD(TMP + k) = LD(TMP + bc); LD(TMP + bc) = t; }
        const double piv = LD(MAT + k * 9 + k);
        for (int c = 0; c < 9; ++c) LD(MAT + k * 9 + c) = LD(MAT + k * 9 + c) / piv;
        for (int r = 0; r < 5; ++r) {
            if (r == k) continue;
            const double f = LD(MAT + r * 9 + k);
            for (int c = 0; c < 9; ++c) LD(MAT + r * 9 + c) = LD(MAT + r * 9 + c) - f * LD(MAT + k * 9 + c);
        }
    }
    zero(sh, BAS, 36);
    for (int j = 0; j < 4; ++j) {
        LD(BAS + j * 9 + (int)LD(TMP + 5 + j)) = 1.0;
        for (int i = 0; i < 5; ++i) LD(BAS + j * 9 + (int)LD(TMP + i)) = -LD(MAT + i * 9 + 5 + j);
    }
    // ---- the ten cubic constraints: det E, then the nine entries of (E E^T - tr(E E^T) / 2) E
    zero(sh, MAT, 200);
    for (int j = 0; j < 3; ++j) {      // det E along the first row: the cofactor of E[0][j] in TMP + 20
        const int c0 = j == 0 ? 1 : 0, c1 = j == 2 ? 1 : 2;
        zero(sh, TMP, 30);
        acc11(sh, TMP, 3 + c0, 6 + c1);
        acc11(sh, TMP + 10, 3 + c1, 6 + c0);
        for (int i = 0; i < 10; ++i) LD(TMP + 20 + i) = LD(TMP + i) - LD(TMP + 10 + i);
        acc21(sh, MAT, TMP + 20, j, j == 1 ? -1.0 : 1.0);
    }
    zero(sh, TMP + 30, 10);      // half the trace of E E^T
    for (int d = 0; d < 3; ++d)
        for (int m = 0; m < 3; ++m) acc11(sh, TMP + 30, 3 * d + m, 3 * d + m);
    for (int i = 0; i < 10; ++i) LD(TMP + 30 + i) = 0.5 * LD(TMP + 30 + i);
    for (int i = 0; i < 3; ++i) {
        zero(sh, TMP, 30);
        for (int k = 0; k < 3; ++k)
            for (int m = 0; m < 3; ++m) acc11(sh, TMP + k * 10, 3 * i + m, 3 * k + m);
        for (int e = 0; e < 10; ++e) LD(TMP + i * 10 + e) = LD(TMP + i * 10 + e) - LD(TMP + 30 + e);
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) acc21(sh, MAT + (1 + 3 * i + j) * 20, TMP + k * 10, 3 * k + j, 1.0);
    }
    // ---- Gauss-Jordan with partial pivoting over the first ten columns
    for (int k = 0; k < 10; ++k) {
        double best = -1.0;
        int br = k;
        for (int r = k; r < 10; ++r) {
            const double a = fabs(LD(MAT + r * 20 + k));
            if (a > best) { best = a; br = r; }
        }
        ok = ok && best > 1e-300;
        for (int c = 0; c < 20; ++c) { const double t = LD(MAT + k * 20 + c); LD(MAT + k * 20 + c) = LD(MAT + br * 20 + c); LD(MAT + br * 20 + c) = t; }
        const double piv = LD(MAT + k * 20 + k);
        for (int c = 0; c < 20; ++c) LD(MAT + k * 20 + c) = LD(MAT + k * 20 + c) / piv;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = LD(MAT + r * 20 + k);
            for (int c = 0; c < 20; ++c) LD(MAT + r * 20 + c) = LD(MAT + r * 20 + c) - f * LD(MAT + k * 20 + c);
        }
    }
    // ---- B(z): rows (4, 5), (6, 7), (8, 9) combined as a - z b, each x p(z) + y q(z) + r(z); written over the dead rows 0 .. 1
    for (int k = 0; k < 3; ++k) {
        const int a = MAT + (4 + 2 * k) * 20 + 10, b = MAT + (5 + 2 * k) * 20 + 10, o = BZ + k * 13;
        LD(o + 0) = LD(a + 2); LD(o + 1) = LD(a + 1) - LD(b + 2); LD(o + 2) = LD(a + 0) - LD(b + 1); LD(o + 3) = -LD(b + 0);
        LD(o + 4) = LD(a + 5); LD(o + 5) = LD(a + 4) - LD(b + 5); LD(o + 6) = LD(a + 3) - LD(b + 4); LD(o + 7) = -LD(b + 3);
        LD(o + 8) = LD(a + 9); LD(o + 9) = LD(a + 8) - LD(b + 9); LD(o + 10) = LD(a + 7) - LD(b + 8); LD(o + 11) = LD(a + 6) - LD(b + 7);
        LD(o + 12) = -LD(b + 6);
    }
    // ---- det B(z), degree 10, into the chain's first row; the minors of rows 1, 2 in TMP
    {
        const int p0 = BZ, q0 = BZ + 4, r0 = BZ + 8, p1 = BZ + 13, q1 = BZ + 17, r1 = BZ + 21, p2 = BZ + 26, q2 = BZ + 30, r2 = BZ + 34;
        const int mq = TMP, mp = TMP + 8, mr = TMP + 16;
        zero(sh, TMP, 23);
        acc_conv(sh, mq, q1, 4, r2, 5, 1.0); acc_conv(sh, mq, q2, 4, r1, 5, -1.0);
        acc_conv(sh, mp, p1, 4, r2, 5, 1.0); acc_conv(sh, mp, p2, 4, r1, 5, -1.0);
        acc_conv(sh, mr, p1, 4, q2, 4, 1.0); acc_conv(sh, mr, p2, 4, q1, 4, -1.0);
        zero(sh, CHAIN, 121);
        acc_conv(sh, CHAIN, p0, 4, mq, 8, 1.0); acc_conv(sh, CHAIN, q0, 4, mp, 8, -1.0); acc_conv(sh, CHAIN, r0, 5, mr, 7, 1.0);
    }
    double big = 0.0;
    for (int i = 0; i < 11; ++i) big = fmax(big, fabs(LD(CHAIN + i)));
    for (int i = 0; i < 11; ++i) LD(CHAIN + i) = LD(CHAIN + i) / big;
    double bound = 0.0;
    for (int i = 0; i < 10; ++i) bound = fmax(bound, fabs(LD(CHAIN + i) / LD(CHAIN + 10)));
    bound = 1.0 + bound;      // Cauchy: every root lies inside
    // ---- the Sturm chain: S1 = S0', S(k+1) = -rem(S(k-1), S(k)), every remainder divided by its largest magnitude
    for (int i = 1; i < 11; ++i) LD(CHAIN + 11 + i - 1) = (double)i * LD(CHAIN + i);
    bool chain_ok = true;
    for (int k = 1; k < 10; ++k) {
        const int nd = 11 - k, a = CHAIN + (k - 1) * 11, b = CHAIN + k * 11, o = CHAIN + (k + 1) * 11;
        const double q1 = LD(a + nd) / LD(b + nd - 1);
        const double q0 = (LD(a + nd - 1) - q1 * LD(b + nd - 2)) / LD(b + nd - 1);
        double s = 0.0;
        for (int i = 0; i < nd - 1; ++i) {
            const double r = (LD(a + i) - (i > 0 ? q1 * LD(b + i - 1) : 0.0)) - q0 * LD(b + i);
            LD(o + i) = r;
            s = fmax(s, fabs(r));
            chain_ok = chain_ok && fin(r);
        }
        for (int i = 0; i < nd - 1; ++i) { LD(o + i) = -LD(o + i) / s; chain_ok = chain_ok && fin(LD(o + i)); }
    }
    for (int i = 0; i < 22; ++i) chain_ok = chain_ok && fin(LD(CHAIN + i));
    ok = ok && chain_ok && fin(bound);
    if (!ok) { bound = 1.0; zero(sh, CHAIN, 121); }
    const int v_lo = sign_changes(sh, -bound);
    int n_roots = v_lo - sign_changes(sh, bound);
    n_roots = !ok ? 0 : (n_roots < 0 ? 0 : (n_roots > MAX_SOL ? MAX_SOL : n_roots));
    // ---- every real root in ascending order: bisection on the count, Newton on det B(z), (x, y) from the null vector of B(z)
    const size_t slot = (size_t)p * trials + (live ? tr : 0);
    double* out = Es + slot * (MAX_SOL * 9);
    if (live)
        for (int e = 0; e < MAX_SOL * 9; ++e) out[e] = 0.0;
    int ns = 0;
    for (int k = 1; k <= MAX_SOL; ++k) {
        if (__ballot(k <= n_roots) == 0ull) break;      // uniform: no lane of the wave has a k-th root
        double lo = -bound, hi = bound;
        for (int it = 0; it < BISECT; ++it) {
            const double mid = 0.5 * (lo + hi);
            const bool ge = v_lo - sign_changes(sh, mid) >= k;
            hi = ge ? mid : hi;
            lo = ge ? lo : mid;
        }
        double z = 0.5 * (lo + hi);
        V3 b0, b1, b2, d0, d1, d2;
        for (int it = 0; it < NEWTON; ++it) {
            bz_row(sh, 0, z, b0, d0); bz_row(sh, 1, z, b1, d1); bz_row(sh, 2, z, b2, d2);
            const double f = det3(b0, b1, b2);
            const double df = (det3(d0, b1, b2) + det3(b0, d1, b2)) + det3(b0, b1, d2);
            const double step = f / df;
            z = fin(step) ? z - step : z;
        }
        bz_row(sh, 0, z, b0, d0); bz_row(sh, 1, z, b1, d1); bz_row(sh, 2, z, b2, d2);
        V3 nv = cross(b0, b1);
        double nn = dot(nv, nv);
        const V3 c02 = cross(b0, b2), c12 = cross(b1, b2);
        if (dot(c02, c02) > nn) { nv = c02; nn = dot(c02, c02); }
        if (dot(c12, c12) > nn) { nv = c12; nn = dot(c12, c12); }
        const double x = nv.x / nv.z, y = nv.y / nv.z;
        double E[9], ss = 0.0;
        bool good = k <= n_roots;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            E[e] = ((x * LD(BAS + e) + y * LD(BAS + 9 + e)) + z * LD(BAS + 18 + e)) + LD(BAS + 27 + e);
            ss += E[e] * E[e];
        }
        const double nrm = sqrt(ss);
#pragma unroll
        for (int e = 0; e < 9; ++e) { E[e] = E[e] / nrm; good = good && fin(E[e]); }
        good = good && nrm > 0.0 && violation(E) <= CHECK_TOL;
        if (good && live) {      // valid roots compacted to the front, in root order
#pragma unroll
            for (int e = 0; e < 9; ++e) out[ns * 9 + e] = E[e];
            ++ns;
        }
    }
    if (live) {
        n_sol[slot] = ns;
        if (fives)
#pragma unroll
            for (int k = 0; k < 5; ++k) fives[slot * 5 + k] = pick[k];
    }
}
#undef LD

// ---------------------------------------------------------------- score: (hypotheses x rows) Sampson tests
// pose_score_kernel's structure: one workgroup per (pair, SCORE_TRIALS trials), the pair's rows through LDS in chunks of SCORE_CHUNK
// (structure of arrays), each wave takes SCORE_TPW trials in turn per chunk, the slots of a trial scored SCORE_HALF at a time from
// registers, lanes striding over the rows.  Slots beyond n_sol hold zeros: 0 / 0, no inlier.
__global__ __launch_bounds__(256) void twoview_score_kernel(const double* __restrict__ norm, const int* __restrict__ frame_off,
                                                            const int* __restrict__ pairs, const int* __restrict__ m_off,
                                                            const int* __restrict__ matches, const int* __restrict__ cam_model,
        const double* __restrict__ cam_params, int n_frames,
                                                            int n_matches, const double* __restrict__ Es, const int* __restrict__ n_sol,
                                                            int trials, double max_error, int* __restrict__ h_inl, double* __restrict__ h_res) {
    __shared__ double rows[4][SCORE_CHUNK];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tr0 = blockIdx.x * SCORE_TRIALS + wave * SCORE_TPW;
    const PairRows g = pair_rows(norm, frame_off, pairs, m_off, matches, n_frames, n_matches, p);
    double thr2 = 0.0;
    if (g.ok) {
        const int f0 = pairs[(size_t)p * 2], f1 = pairs[(size_t)p * 2 + 1];
        const double th = max_error * pixel_unit(cam_model, cam_params, f0, f1);
        thr2 = th * th;
    }
    int cnt[SCORE_TPW][MAX_SOL];
    double res[SCORE_TPW][MAX_SOL];
#pragma unroll
    for (int t = 0; t < SCORE_TPW; ++t)
#pragma unroll
        for (int k = 0; k < MAX_SOL; ++k) { cnt[t][k] = 0; res[t][k] = 0.0; }
    for (int c0 = 0; c0 < g.n; c0 += SCORE_CHUNK) {
        const int len = g.n - c0 < SCORE_CHUNK ? g.n - c0 : SCORE_CHUNK;
        __syncthreads();
        for (int i = tid; i < len; i += 256) load_row(g, c0 + i, rows[0][i], rows[1][i], rows[2][i], rows[3][i]);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < SCORE_TPW; ++t) {
            if (tr0 + t >= trials) continue;      // uniform over the wave
            const double* es = Es + ((size_t)p * trials + tr0 + t) * (MAX_SOL * 9);
#pragma unroll
            for (int h = 0; h < MAX_SOL; h += SCORE_HALF) {
                double E[SCORE_HALF][9];
#pragma unroll
                for (int k = 0; k < SCORE_HALF; ++k)
#pragma unroll
                    for (int e = 0; e < 9; ++e) E[k][e] = es[(h + k) * 9 + e];
                for (int i = lane; i < len; i += 64) {
                    const double u0 = rows[0][i], v0 = rows[1][i], u1 = rows[2][i], v1 = rows[3][i];
#pragma unroll
                    for (int k = 0; k < SCORE_HALF; ++k) {
                        const double e = sampson(E[k], u0, v0, u1, v1);
                        const bool in = e <= thr2;      // NaN compares false
                        cnt[t][h + k] += in;
                        res[t][h + k] += in ? e : 0.0;
                    }
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
        for (int k = 0; k < MAX_SOL; ++k) {
            const int c = wave_sum_i32(cnt[t][k]);
            const double s = wave_sum_f64(res[t][k]);
            if (lane == 0) {
                h_inl[slot * MAX_SOL + k] = k < ns ? c : -1;      // -1 = no hypothesis in this slot
                h_res[slot * MAX_SOL + k] = k < ns ? s : 0.0;
            }
        }
    }
}

// ---------------------------------------------------------------- finish: decomposition, refinement, the outputs of a pair
using Rel = Pose;      // frame 1 from frame 0, |t| = 1

struct FinishShared {
    LmState<Rel, LM_VALS> lm;
    Rel more[3];      // with lm.cand the four of the decomposition, before the refinement takes lm.cand for its candidate
    int sred[4];
    int wsum[4];
    __device__ Rel& cand(int k) { return k == 0 ? lm.cand : more[k - 1]; }
};

__device__ __forceinline__ void essential_of(const Rel& q, double* E) {      // [t]x R / sqrt(2): Frobenius norm 1
    const double s = sqrt(2.0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        E[c] = (q.t[1] * q.R[6 + c] - q.t[2] * q.R[3 + c]) / s;
        E[3 + c] = (q.t[2] * q.R[c] - q.t[0] * q.R[6 + c]) / s;
        E[6 + c] = (q.t[0] * q.R[3 + c] - q.t[1] * q.R[c]) / s;
    }
}

// The four (R, t) of a Frobenius-normalised E: t the largest cross product of two columns, normalised; R = cof(E') -+ [t]x E' with
// E' = sqrt(2) E (Horn 1990), then Gram-Schmidt with the third row the cross product of the first two: det R = +1.
__device__ void decompose(const double* __restrict__ E, FinishShared& sh) {
    const V3 c0 = {E[0], E[3], E[6]}, c1 = {E[1], E[4], E[7]}, c2 = {E[2], E[5], E[8]};
    V3 b = cross(c0, c1);
    double bn = dot(b, b);
    const V3 b02 = cross(c0, c2), b12 = cross(c1, c2);
    if (dot(b02, b02) > bn) { b = b02; bn = dot(b02, b02); }
    if (dot(b12, b12) > bn) { b = b12; bn = dot(b12, b12); }
    const double nb = sqrt(bn);
    const V3 t = {b.x / nb, b.y / nb, b.z / nb};
    const double s = sqrt(2.0);
    const V3 r0 = {E[0] * s, E[1] * s, E[2] * s}, r1 = {E[3] * s, E[4] * s, E[5] * s}, r2 = {E[6] * s, E[7] * s, E[8] * s};
    const V3 cf[3] = {cross(r1, r2), cross(r2, r0), cross(r0, r1)};
    // [t]x E'
    double tE[9];
    const double Es_[9] = {r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z};
    for (int c = 0; c < 3; ++c) {
        tE[c] = t.y * Es_[6 + c] - t.z * Es_[3 + c];
        tE[3 + c] = t.z * Es_[c] - t.x * Es_[6 + c];
        tE[6 + c] = t.x * Es_[3 + c] - t.y * Es_[c];
    }
    for (int v = 0; v < 2; ++v) {
        const double sg = v == 0 ? -1.0 : 1.0;
        V3 a0 = {cf[0].x + sg * tE[0], cf[0].y + sg * tE[1], cf[0].z + sg * tE[2]};
        V3 a1 = {cf[1].x + sg * tE[3], cf[1].y + sg * tE[4], cf[1].z + sg * tE[5]};
        const double n0 = sqrt(dot(a0, a0));
        a0 = {a0.x / n0, a0.y / n0, a0.z / n0};
        const double d = dot(a1, a0);
        a1 = {a1.x - d * a0.x, a1.y - d * a0.y, a1.z - d * a0.z};
        const double n1 = sqrt(dot(a1, a1));
        a1 = {a1.x / n1, a1.y / n1, a1.z / n1};
        const V3 a2 = cross(a0, a1);
        for (int w = 0; w < 2; ++w) {
            Rel& q = sh.cand(v * 2 + w);
            q.R[0] = a0.x; q.R[1] = a0.y; q.R[2] = a0.z; q.R[3] = a1.x; q.R[4] = a1.y; q.R[5] = a1.z; q.R[6] = a2.x; q.R[7] = a2.y; q.R[8] = a2.z;
            const double ts = w == 0 ? 1.0 : -1.0;
            q.t[0] = ts * t.x; q.t[1] = ts * t.y; q.t[2] = ts * t.z;
        }
    }
}

// positive depth in both frames: lam0 from x1 x (lam0 R x0 + t) = 0, lam1 = (lam0 R x0 + t) . x1 / |x1|^2
__device__ __forceinline__ bool in_front(const Rel& q, double u0, double v0, double u1, double v1) {
    const V3 y = {(q.R[0] * u0 + q.R[1] * v0) + q.R[2], (q.R[3] * u0 + q.R[4] * v0) + q.R[5], (q.R[6] * u0 + q.R[7] * v0) + q.R[8]};
    const V3 x1 = {u1, v1, 1.0}, t = {q.t[0], q.t[1], q.t[2]};
    const V3 a = cross(x1, y), b = cross(x1, t);
    const double lam0 = -dot(a, b) / dot(a, a);
    const V3 z = {lam0 * y.x + t.x, lam0 * y.y + t.y, lam0 * y.z + t.z};
    const double lam1 = dot(z, x1) / dot(x1, x1);
    return lam0 > 0.0 && lam1 > 0.0;
}

// marks the Sampson inliers of E (one byte per match, thread tid owns matches tid, tid + 256, ...) and returns their number
__device__ int mark_inliers(const double* __restrict__ E, const PairRows& g, double thr2, unsigned char* __restrict__ mask, int* sred) {
    int c = 0;
    for (int i = threadIdx.x; i < g.n; i += 256) {
        double u0, v0, u1, v1;
        load_row(g, i, u0, v0, u1, v1);
        const bool in = sampson(E, u0, v0, u1, v1) <= thr2;
        mask[i] = in;
        c += in;
    }
    return block_sum_i32<4>(c, sred);
}

__device__ int count_front(const Rel& q, const PairRows& g, const unsigned char* __restrict__ mask, int* sred) {
    int c = 0;
    for (int i = threadIdx.x; i < g.n; i += 256) {
        if (!mask[i]) continue;
        double u0, v0, u1, v1;
        load_row(g, i, u0, v0, u1, v1);
        c += in_front(q, u0, v0, u1, v1);
    }
    return block_sum_i32<4>(c, sred);
}

// two unit vectors that span the tangent plane of the sphere at t: along t x (the axis where |t| is smallest), and t x that
__device__ __forceinline__ void tangent_basis(const double* t, V3& b1, V3& b2) {
    int a = 0;
    if (fabs(t[1]) < fabs(t[a])) a = 1;
    if (fabs(t[2]) < fabs(t[a])) a = 2;
    const V3 tv = {t[0], t[1], t[2]}, e = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
    const V3 c = cross(tv, e);
    const double n = sqrt(dot(c, c));
    b1 = {c.x / n, c.y / n, c.z / n};
    b2 = cross(tv, b1);
}

__device__ __forceinline__ void skew_times(V3 v, const double* __restrict__ R, double* out) {      // [v]x R
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[c] = v.y * R[6 + c] - v.z * R[3 + c];
        out[3 + c] = v.z * R[c] - v.x * R[6 + c];
        out[6 + c] = v.x * R[3 + c] - v.y * R[c];
    }
}

// cost, J^T W J, J^T W r of sum log(1 + (d / scale)^2), d the signed Sampson distance, over the masked matches at q -> tot[LM_VALS]
__device__ void lm_pass(const Rel& q, const PairRows& g, const unsigned char* __restrict__ mask, double scale, double (*wred)[LM_VALS], double* tot) {
    double E[9], dE[5][9];
    const V3 tv = {q.t[0], q.t[1], q.t[2]};
    skew_times(tv, q.R, E);
    V3 b1, b2;
    tangent_basis(q.t, b1, b2);
#pragma unroll
    for (int k = 0; k < 3; ++k) {      // d / d omega_k: [t]x [e_k]x R
        double eR[9];
        const V3 ek = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        skew_times(ek, q.R, eR);
        skew_times(tv, eR, dE[k]);
    }
    skew_times(b1, q.R, dE[3]);
    skew_times(b2, q.R, dE[4]);
    double acc[LM_VALS];
#pragma unroll
    for (int e = 0; e < LM_VALS; ++e) acc[e] = 0.0;
    for (int i = threadIdx.x; i < g.n; i += 256) {
        if (!mask[i]) continue;
        double u0, v0, u1, v1;
        load_row(g, i, u0, v0, u1, v1);
        const double a0 = (E[0] * u0 + E[1] * v0) + E[2], a1 = (E[3] * u0 + E[4] * v0) + E[5], a2 = (E[6] * u0 + E[7] * v0) + E[8];
        const double b0 = (E[0] * u1 + E[3] * v1) + E[6], b1_ = (E[1] * u1 + E[4] * v1) + E[7];
        const double c = (u1 * a0 + v1 * a1) + a2;
        const double den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1_ * b1_;
        const double sq = sqrt(den);
        const double r = c / sq / scale;
        double J[5];
        bool okr = fin(r);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double* D = dE[k];
            const double da0 = (D[0] * u0 + D[1] * v0) + D[2], da1 = (D[3] * u0 + D[4] * v0) + D[5], da2 = (D[6] * u0 + D[7] * v0) + D[8];
            const double db0 = (D[0] * u1 + D[3] * v1) + D[6], db1 = (D[1] * u1 + D[4] * v1) + D[7];
            const double dc = (u1 * da0 + v1 * da1) + da2;
            const double dd = 2.0 * (((a0 * da0 + a1 * da1) + b0 * db0) + b1_ * db1);
            J[k] = (dc / sq - 0.5 * c * dd / (den * sq)) / scale;
            okr = okr && fin(J[k]);
        }
        if (!okr) continue;
        const double s = r * r;
        const double w = 1.0 / (1.0 + s);      // Cauchy: rho(s) = log(1 + s), rho' = 1 / (1 + s)
        acc[0] += log1p(s);
        int e = 1;
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int c2 = a; c2 < 5; ++c2) acc[e++] += w * (J[a] * J[c2]);
#pragma unroll
        for (int a = 0; a < 5; ++a) acc[16 + a] += w * (J[a] * r);
    }
    block_fold_f64<LM_VALS>(acc, wred, tot);
}

// R <- exp([w]x) R, t <- (t + d3 b1 + d4 b2) normalised
__device__ void rel_update(const Rel& q, const double* __restrict__ d, Rel& o) {
    rot_exp_left(d, q.R, o.R);
    V3 b1, b2;
    tangent_basis(q.t, b1, b2);
    const double t0 = (q.t[0] + d[3] * b1.x) + d[4] * b2.x, t1 = (q.t[1] + d[3] * b1.y) + d[4] * b2.y, t2 = (q.t[2] + d[3] * b1.z) + d[4] * b2.z;
    const double n = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    o.t[0] = t0 / n; o.t[1] = t1 / n; o.t[2] = t2 / n;
}

__global__ __launch_bounds__(256) void twoview_finish_kernel(const double* __restrict__ norm, const int* __restrict__ frame_off,
                                                             const int* __restrict__ pairs, const int* __restrict__ m_off,
                                                             const int* __restrict__ matches, const int* __restrict__ cam_model,
        const double* __restrict__ cam_params, int n_frames,
                                                             int n_matches, const double* __restrict__ Es, const int* __restrict__ h_inl,
                                                             const int* __restrict__ best, int trials, double max_error,
                                                             double min_inlier_ratio, int min_num_inliers, int iters, double* __restrict__ E_out,
                                                             double* __restrict__ qvec, double* __restrict__ tvec, int* __restrict__ num_inliers,
                                                             int* __restrict__ num_front, int* __restrict__ success,
                                                             unsigned char* __restrict__ keep, int* __restrict__ kept, int* __restrict__ edges,
                                                             int* __restrict__ count) {
    __shared__ FinishShared sh;
    const int p = blockIdx.x, tid = threadIdx.x;
    const PairRows g = pair_rows(norm, frame_off, pairs, m_off, matches, n_frames, n_matches, p);
    unsigned char* mask = keep + g.m0;
    const int bi = g.ok && g.n >= 5 ? best[p] : -1;
    bool good = bi >= 0;      // uniform
    double Ef[9];
    Rel q;
    int support = 0, front = 0;
#pragma unroll
    for (int a = 0; a < 9; ++a) Ef[a] = 0.0;
    if (good) {
        const int f0 = pairs[(size_t)p * 2], f1 = pairs[(size_t)p * 2 + 1];
        const double unit = pixel_unit(cam_model, cam_params, f0, f1);
        const double th = max_error * unit, thr2 = th * th, scale = 1.0 * unit;
        const int n0 = h_inl[(size_t)p * trials * MAX_SOL + bi];
        double Eh[9];
#pragma unroll
        for (int a = 0; a < 9; ++a) Eh[a] = Es[((size_t)p * trials * MAX_SOL + bi) * 9 + a];
        mark_inliers(Eh, g, thr2, mask, sh.sred);
        // the (R, t) among the four with most inliers in front of both cameras, the lowest index on a tie
        if (tid == 0) decompose(Eh, sh);
        __syncthreads();
        int bf = -1, bk = 0;
        for (int k = 0; k < 4; ++k) {
            const Rel c = sh.cand(k);
            const int f = count_front(c, g, mask, sh.sred);
            if (f > bf) { bf = f; bk = k; }
        }
        const Rel h = sh.cand(bk);
        __syncthreads();      // lm.cand is the refinement's candidate from here on
        good = pose_finite(h);
        if (good) {
            // `iters` Levenberg-Marquardt iterations from q on the masked matches; every thread ends with the same model.  The
            // 5 x 5 normal equations go through chol_solve6 with the sixth unknown pinned (H66 = 1, g6 = 0).
            const auto pass = [&](const Rel& m) { lm_pass(m, g, mask, scale, sh.lm.wred, sh.lm.tot); };
            const auto step = [](const double* cur, double lam, const Rel& from, Rel& cand) {
                double H6[21], g6[6], d[6];
                int e6 = 0, e5 = 1;
                for (int a = 0; a < 6; ++a)
                    for (int c = a; c < 6; ++c) H6[e6++] = (a < 5 && c < 5) ? cur[e5++] : (a == 5 ? 1.0 : 0.0);
                for (int a = 0; a < 5; ++a) g6[a] = cur[16 + a];
                g6[5] = 0.0;
                const bool okd = chol_solve6(H6, g6, lam, d);
                if (okd) rel_update(from, d, cand);
                return okd;
            };
            q = h;
            lm_refine(q, iters, sh.lm, pass, step);
            double Er[9];
            essential_of(q, Er);
            mark_inliers(Er, g, thr2, mask, sh.sred);
            lm_refine(q, iters, sh.lm, pass, step);
            essential_of(q, Er);
            support = mark_inliers(Er, g, thr2, mask, sh.sred);
            if (support < n0 || !pose_finite(q)) {      // the refined model lost support: the hypothesis stands
                q = h;
                support = mark_inliers(Eh, g, thr2, mask, sh.sred);
#pragma unroll
                for (int a = 0; a < 9; ++a) Ef[a] = Eh[a];
            } else {
#pragma unroll
                for (int a = 0; a < 9; ++a) Ef[a] = Er[a];
            }
            front = count_front(q, g, mask, sh.sred);
            const double need = fmax((double)min_num_inliers, min_inlier_ratio * (double)g.n);
            good = (double)support >= need;
        }
    }
    // ---- the outputs: zeros for a failed pair, which keeps no match
    if (tid == 0) {
        double qv[4] = {0.0, 0.0, 0.0, 0.0};
        if (good) rot_to_qvec(q.R, qv);
        for (int a = 0; a < 9; ++a) E_out[(size_t)p * 9 + a] = good ? Ef[a] : 0.0;
        for (int a = 0; a < 4; ++a) qvec[(size_t)p * 4 + a] = qv[a];
        for (int a = 0; a < 3; ++a) tvec[(size_t)p * 3 + a] = good ? q.t[a] : 0.0;
        num_inliers[p] = good ? support : 0;
        num_front[p] = good ? front : 0;
        success[p] = good;
    }
    // pram_tri_verify's layout: the mask, the kept matches in their original order from match_off[p] on, the rows they join
    int base = 0;
    for (int c0 = 0; c0 < g.n; c0 += 256) {
        const int i = c0 + tid;
        bool k = false;
        int i0 = -1, i1 = -1;
        if (i < g.n) {
            const size_t e = (size_t)(g.m0 + i);
            i0 = matches[e * 2]; i1 = matches[e * 2 + 1];
            k = good && mask[i];      // a marked match has both indices inside its frame
            keep[e] = k;
            edges[e * 2] = k ? g.r0 + i0 : -1; edges[e * 2 + 1] = k ? g.r1 + i1 : -1;
        }
        int total;
        const int o = chunk_offset<4>(k, sh.wsum, total);
        if (k) { kept[(size_t)(g.m0 + base + o) * 2] = i0; kept[(size_t)(g.m0 + base + o) * 2 + 1] = i1; }
        base += total;
    }
    if (tid == 0) count[p] = base;
}

bool sizes_ok(int n_frames, int n_pairs, int n_matches, int trials) {
    return n_frames >= 0 && n_pairs >= 0 && n_pairs <= 65535 && n_matches >= 0 && trials >= 1 && trials <= (1 << 20);
}

}  // namespace

extern "C" int pram_twoview_hypotheses(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* matches,
                                       int n_frames, int n_pairs, int n_matches, int first_pair, int trials, unsigned long long seed,
                                       double* E, int* n_sol, int* fives, void* stream) {
    PRAM_REQUIRE(norm && frame_off && pairs && match_off && matches && E && n_sol, "pram_twoview_hypotheses: null pointer");
    PRAM_REQUIRE(aligned(norm, 8) && aligned(frame_off, 4) && aligned(pairs, 4) && aligned(match_off, 4) && aligned(matches, 4) && aligned(E, 8) &&
                 aligned(n_sol, 4) && aligned(fives, 4), "pram_twoview_hypotheses: misaligned pointer");
    PRAM_REQUIRE(sizes_ok(n_frames, n_pairs, n_matches, trials) && first_pair >= 0,
                 "pram_twoview_hypotheses: needs n_frames >= 0, 0 <= n_pairs <= 65535, n_matches >= 0, first_pair >= 0, 1 <= trials <= 2^20");
    if (n_pairs == 0) return PRAM_OK;
    opt_in_lds<twoview_hypotheses_kernel>(HYP_LDS);
    hipLaunchKernelGGL(twoview_hypotheses_kernel, dim3(cdiv(trials, HYP_LANES), n_pairs), dim3(HYP_LANES), HYP_LDS, (hipStream_t)stream, norm,
                       frame_off, pairs, match_off, matches, n_frames, n_matches, first_pair, trials, seed, E, n_sol, fives);
    return pram_launch_status("pram_twoview_hypotheses");
}

extern "C" int pram_twoview_score(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* matches,
                                  const int* cam_model, const double* cam_params, int n_frames, int n_pairs, int n_matches, const double* E, const int* n_sol,
                                  int trials, double max_error, int* h_inliers, double* h_resid, int* best, void* stream) {
    PRAM_REQUIRE(norm && frame_off && pairs && match_off && matches && cam_model && cam_params && E && n_sol && h_inliers && h_resid && best,
                 "pram_twoview_score: null pointer");
    PRAM_REQUIRE(aligned(norm, 8) && aligned(frame_off, 4) && aligned(pairs, 4) && aligned(match_off, 4) && aligned(matches, 4) &&
                 aligned(cam_model, 4) && aligned(cam_params, 8) && aligned(E, 8) && aligned(n_sol, 4) && aligned(h_inliers, 4) && aligned(h_resid, 8) && aligned(best, 4),
                 "pram_twoview_score: misaligned pointer");
    PRAM_REQUIRE(sizes_ok(n_frames, n_pairs, n_matches, trials) && max_error > 0.0,
                 "pram_twoview_score: needs n_frames >= 0, 0 <= n_pairs <= 65535, n_matches >= 0, 1 <= trials <= 2^20, max_error > 0");
    if (n_pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(twoview_score_kernel, dim3(cdiv(trials, SCORE_TRIALS), n_pairs), dim3(256), 0, (hipStream_t)stream, norm, frame_off, pairs,
                       match_off, matches, cam_model, cam_params, n_frames, n_matches, E, n_sol, trials, max_error, h_inliers, h_resid);
    hipLaunchKernelGGL(ransac_pick_kernel, dim3(n_pairs), dim3(256), 0, (hipStream_t)stream, h_inliers, h_resid, trials * MAX_SOL, best);
    return pram_launch_status("pram_twoview_score");
}

extern "C" int pram_twoview_finish(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* matches,
                                   const int* cam_model, const double* cam_params, int n_frames, int n_pairs, int n_matches, const double* E, const int* h_inliers,
                                   const int* best, int trials, double max_error, double min_inlier_ratio, int min_num_inliers,
                                   int refine_iters, double* E_out, double* qvec, double* tvec, int* num_inliers, int* num_front,
                                   int* success, unsigned char* keep, int* kept, int* edges, int* count, void* stream) {
    PRAM_REQUIRE(norm && frame_off && pairs && match_off && matches && cam_model && cam_params && E && h_inliers && best && E_out && qvec && tvec && num_inliers &&
                 num_front && success && keep && kept && edges && count, "pram_twoview_finish: null pointer");
    PRAM_REQUIRE(aligned(norm, 8) && aligned(frame_off, 4) && aligned(pairs, 4) && aligned(match_off, 4) && aligned(matches, 4) &&
                 aligned(cam_model, 4) && aligned(cam_params, 8) && aligned(E, 8) && aligned(h_inliers, 4) && aligned(best, 4) && aligned(E_out, 8) && aligned(qvec, 8) &&
                 aligned(tvec, 8) && aligned(num_inliers, 4) && aligned(num_front, 4) && aligned(success, 4) && aligned(kept, 4) &&
                 aligned(edges, 4) && aligned(count, 4), "pram_twoview_finish: misaligned pointer");
    PRAM_REQUIRE(sizes_ok(n_frames, n_pairs, n_matches, trials) && max_error > 0.0 && min_inlier_ratio >= 0.0 && min_num_inliers >= 0 &&
                 refine_iters >= 0 && refine_iters <= 1000,
                 "pram_twoview_finish: needs n_frames >= 0, 0 <= n_pairs <= 65535, n_matches >= 0, 1 <= trials <= 2^20, max_error > 0, "
                 "min_inlier_ratio >= 0, min_num_inliers >= 0, 0 <= refine_iters <= 1000");
    if (n_pairs == 0) return PRAM_OK;
    hipLaunchKernelGGL(twoview_finish_kernel, dim3(n_pairs), dim3(256), 0, (hipStream_t)stream, norm, frame_off, pairs, match_off, matches, cam_model,
                       cam_params, n_frames, n_matches, E, h_inliers, best, trials, max_error, min_inlier_ratio, min_num_inliers, refine_iters, E_out, qvec,
                       tvec, num_inliers, num_front, success, keep, kept, edges, count);
    return pram_launch_status("pram_twoview_finish");
}
