// K-means labelling of a map's points: what RecMap.cluster(method='kmeans') of the reference (recognition/recmap.py:85-122) takes
// from sklearn's KMeans(n_clusters=k, random_state=0), on the points as the host centred them.
//   * seeding: sklearn's k-means++ with the host's random numbers.  Per step three launches: one workgroup picks the winner of
//     the previous step's candidates and the block every new target falls into; every block takes the new seed into `closest` and
//     the blocks the targets fall into walk to their candidates; every block adds up every candidate's potential.
//   * Lloyd iterations: four launches each (assignment; cluster sums per block; block partials in block order; one workgroup that
//     relocates empty clusters, divides, measures the shift and decides).  A `done` word makes later iterations return at once.
// One order for every floating-point sum (include/pram_hip.h): inside a block of PRAM_KMEANS_BLOCK points the terms are added to 0.0
// in ascending index, the block partials are added to 0.0 in ascending block index.  That makes the sums inside a block serial: one
// thread walks an LDS row, which is what the restatement (tests/kmeans_ref.py) does and why the two agree bit for bit.  Float64
// throughout, every product and sum written out (the library is built with -ffp-contract=off); no floating-point atomics; plain
// stores only; every index read from memory is checked against the size given beside it; no workgroup waits for another.
#include "glue.h"

namespace {

constexpr int KB = PRAM_KMEANS_BLOCK, KMAX = PRAM_KMEANS_MAX_K, TMAX = PRAM_KMEANS_MAX_TRIALS;
constexpr int KC = 512;        // centres per LDS chunk of the assignment: three rows of 512 doubles, 12 KB
constexpr int SUB = 256;       // points of a block per pass of the 256-thread kernels
constexpr int ROW = SUB + 1;   // LDS row stride in doubles: the serial readers of neighbouring rows fall into different banks
static_assert(KB == 1024 && KB % SUB == 0, "the cluster sums run one thread per point of a block, the other kernels whole passes");
static_assert(KMAX == 4096, "the stable rank of the cluster sums compares 12 label bits; four histogram entries per thread");
enum { ST_DONE = 0, ST_ITER, ST_STRICT, ST_RELOC, ST_CHANGED };
static_assert(ST_CHANGED < PRAM_KMEANS_STATE_WORDS, "state words");

__device__ __forceinline__ double dist2(double x0, double x1, double x2, double c0, double c1, double c2) {
    const double a = x0 - c0, b = x1 - c1, c = x2 - c2;
    return (a * a + b * b) + c * c;
}

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// ---------------------------------------------------------------------------------------------------------------- assignment
// One thread per point, the centres through LDS as a structure of arrays (every lane reads the same word: a broadcast), the best
// index and distance in registers.  MODE 0: the public step.  MODE 1: iteration `iter`, labels into the buffer of its parity; a
// label that differs from the other buffer's raises the changed word.  MODE 2: the finish: after strict convergence the labels
// stand and only the distance to the point's own (moved) centre is taken.
template <int MODE>
__global__ __launch_bounds__(256) void km_assign_kernel(const double* __restrict__ x, int n, const double* __restrict__ centers, int k,
                                                        int* __restrict__ labels_out, double* __restrict__ dist, int* __restrict__ labels2,
                                                        int iter, int* __restrict__ state) {
    __shared__ double sc[3][KC];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    const bool on = i < n;
    int* out = labels_out;
    const int* prev = nullptr;
    if (MODE == 1) {
        if (state[ST_DONE] != 0) return;
        out = labels2 + (size_t)(iter & 1) * n;
        prev = labels2 + (size_t)((iter + 1) & 1) * n;
    }
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (on) { x0 = x[i * 3]; x1 = x[i * 3 + 1]; x2 = x[i * 3 + 2]; }
    if (MODE == 2 && state[ST_STRICT] != 0) {      // uniform
        if (on) {
            int l = labels2[(size_t)((state[ST_ITER] - 1) & 1) * n + i];
            l = (unsigned)l < (unsigned)k ? l : 0;
            out[i] = l;
            dist[i] = dist2(x0, x1, x2, centers[(size_t)l * 3], centers[(size_t)l * 3 + 1], centers[(size_t)l * 3 + 2]);
        }
        return;
    }
    double best = pos_inf();
    int bi = 0;
    for (int c0 = 0; c0 < k; c0 += KC) {
        const int kc = k - c0 < KC ? k - c0 : KC;
        __syncthreads();      // the previous chunk's readers
        for (int j = tid; j < kc; j += 256) {
            sc[0][j] = centers[(size_t)(c0 + j) * 3];
            sc[1][j] = centers[(size_t)(c0 + j) * 3 + 1];
            sc[2][j] = centers[(size_t)(c0 + j) * 3 + 2];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < kc; ++j) {
            const double d = dist2(x0, x1, x2, sc[0][j], sc[1][j], sc[2][j]);
            if (d < best) { best = d; bi = c0 + j; }      // strict: the lowest index keeps a tie
        }
    }
    if (!on) return;
    out[i] = bi;
    dist[i] = best;
    if (MODE == 1 && prev[i] != bi) state[ST_CHANGED] = 1;      // every writer stores the same value
}

// ---------------------------------------------------------------------------------------------------------------- cluster sums
// One workgroup per block, one thread per point.  The block's points are ordered by label, stably: a histogram of the labels
// (integer LDS atomics), its exclusive scan, then wave after wave in ascending order every point takes the place cursor[label] +
// (the number of lower lanes of its wave with its label).  Then one thread per cluster adds its run in place order, which is
// ascending point index.  part [nb][3][k], cnt [nb][k]: a cluster the block does not hold gets 0.0 and 0.
__global__ __launch_bounds__(KB) void km_block_sums_kernel(const double* __restrict__ x, int n, int k, const int* __restrict__ labels2, int iter,
                                                           double* __restrict__ part, int* __restrict__ cnt, const int* __restrict__ state) {
    __shared__ double xs[3][KB];
    __shared__ int hist[KMAX];
    __shared__ int cursor[KMAX];
    __shared__ int wtot[KB / 64];
    if (state[ST_DONE] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const long long i = (long long)b * KB + tid;
    const int* labels = labels2 + (size_t)(iter & 1) * n;
    for (int c = tid; c < k; c += KB) hist[c] = 0;
    __syncthreads();
    int l = -1;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (i < n) {
        l = labels[i];
        if ((unsigned)l >= (unsigned)k) l = -1;
        x0 = x[i * 3]; x1 = x[i * 3 + 1]; x2 = x[i * 3 + 2];
    }
    const bool valid = l >= 0;
    if (valid) atomicAdd(&hist[l], 1);
    __syncthreads();
    // exclusive scan of the histogram: four clusters to a thread, a scan over the lanes, the waves' totals through LDS
    int h[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = tid * 4 + q;
        h[q] = c < k ? hist[c] : 0;
        s += h[q];
    }
    int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int off = incl - s;
    for (int w = 0; w < wave; ++w) off += wtot[w];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = tid * 4 + q;
        if (c < k) cursor[c] = off;
        off += h[q];
    }
    // the lanes of this wave that hold the same label, bit by bit of the label
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 12; ++bit) {
        const bool one = ((l >> bit) & 1) != 0;
        const unsigned long long bal = __ballot(valid && one);
        same &= one ? bal : ~bal;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull)), group = __popcll(same);
    for (int w = 0; w < KB / 64; ++w) {
        __syncthreads();      // the cursors of the scan, then of the wave before
        if (wave == w && valid) {
            const int pos = cursor[l] + rank;      // one read instruction for the whole wave, before the group's last lane writes
            if (pos < KB) { xs[0][pos] = x0; xs[1][pos] = x1; xs[2][pos] = x2; }
            if (rank == group - 1) cursor[l] = pos + 1;
        }
    }
    __syncthreads();
    for (int c = tid; c < k; c += KB) {
        int e = cursor[c];
        const int hc = hist[c];
        e = e > KB ? KB : e;
        int p = e - hc;
        p = p < 0 ? 0 : p;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (; p < e; ++p) { a0 += xs[0][p]; a1 += xs[1][p]; a2 += xs[2][p]; }
        part[((size_t)b * 3) * k + c] = a0;
        part[((size_t)b * 3 + 1) * k + c] = a1;
        part[((size_t)b * 3 + 2) * k + c] = a2;
        cnt[(size_t)b * k + c] = hc;
    }
}

// the block partials in ascending block index: one thread per sum (sums [3][k]) and per count
__global__ __launch_bounds__(256) void km_reduce_kernel(const double* __restrict__ part, const int* __restrict__ cnt, int nb, int k,
                                                        double* __restrict__ sums, int* __restrict__ counts, const int* __restrict__ state) {
    if (state[ST_DONE] != 0) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < 3 * k) {
        double a = 0.0;
#pragma unroll 8
        for (int b = 0; b < nb; ++b) a += part[(size_t)b * 3 * k + t];
        sums[t] = a;
    } else if (t < 4 * k) {
        const int c = t - 3 * k;
        int a = 0;
#pragma unroll 8
        for (int b = 0; b < nb; ++b) a += cnt[(size_t)b * k + c];
        counts[c] = a;
    }
}

// One workgroup.  Empty clusters in ascending index each take the next of the points farthest from their own centre (descending
// distance, lowest index on ties: a scan of dist per empty cluster for the first point after the previous pick in that order);
// the point leaves its old cluster's sum and count.  Then the new centres, the shift, and the decision.
__global__ __launch_bounds__(256) void km_update_kernel(const double* __restrict__ x, int n, int k, double* __restrict__ centers,
                                                        double* __restrict__ sums, int* __restrict__ counts, const int* __restrict__ labels2,
                                                        const double* __restrict__ dist, int* __restrict__ empties, int* __restrict__ state,
                                                        double* __restrict__ shift_out, double tol_abs, int max_iter, int iter) {
    __shared__ double terms[KMAX];
    __shared__ double rd[256];
    __shared__ int ri[256];
    __shared__ int wsum[4];
    if (state[ST_DONE] != 0) return;
    const int tid = threadIdx.x;
    const int* labels = labels2 + (size_t)(iter & 1) * n;
    int n_empty = 0;
    for (int c0 = 0; c0 < k; c0 += 256) {
        const int c = c0 + tid;
        const bool f = c < k && counts[c] == 0;
        int total;
        const int o = chunk_offset<4>(f, wsum, total);
        if (f) empties[n_empty + o] = c;
        n_empty += total;
    }
    __syncthreads();
    double pd = 0.0;
    int pi = -1, moved = 0;
    for (int j = 0; j < n_empty && j < k; ++j) {
        double bd = 0.0;
        int bi = -1;
        for (long long i = tid; i < n; i += 256) {
            const double d = dist[i];
            const bool after = pi < 0 || d < pd || (d == pd && i > pi);
            if (after && (bi < 0 || d > bd)) { bd = d; bi = (int)i; }
        }
        rd[tid] = bd;
        ri[tid] = bi;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                const double od = rd[tid + s];
                const int oi = ri[tid + s];
                if (oi >= 0 && (ri[tid] < 0 || od > rd[tid] || (od == rd[tid] && oi < ri[tid]))) { rd[tid] = od; ri[tid] = oi; }
            }
            __syncthreads();
        }
        pi = ri[0];
        pd = rd[0];
        __syncthreads();      // everyone has read the pick before the next round writes
        if (pi < 0) break;      // no point left: uniform
        ++moved;
        if (tid == 0) {
            const int e = empties[j], o = labels[pi];
            const double p0 = x[(size_t)pi * 3], p1 = x[(size_t)pi * 3 + 1], p2 = x[(size_t)pi * 3 + 2];
            if ((unsigned)o < (unsigned)k) {
                sums[o] = sums[o] - p0; sums[k + o] = sums[k + o] - p1; sums[2 * k + o] = sums[2 * k + o] - p2;
                counts[o] -= 1;
            }
            if ((unsigned)e < (unsigned)k) {
                sums[e] = p0; sums[k + e] = p1; sums[2 * k + e] = p2;
                counts[e] = 1;
            }
        }
    }
    __syncthreads();
    for (int c = tid; c < k; c += 256) {
        const int m = counts[c];
        double nv[3], df[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double s = sums[d * k + c];
            nv[d] = m > 0 ? s / (double)m : s;      // a cluster a relocation emptied keeps its sum
            df[d] = nv[d] - centers[(size_t)c * 3 + d];
            centers[(size_t)c * 3 + d] = nv[d];
        }
        terms[c] = (df[0] * df[0] + df[1] * df[1]) + df[2] * df[2];
    }
    __syncthreads();
    if (tid == 0) {
        double sh = 0.0;
#pragma unroll 8
        for (int c = 0; c < k; ++c) sh += terms[c];
        shift_out[0] = sh;
        const int changed = state[ST_CHANGED];
        state[ST_CHANGED] = 0;
        state[ST_ITER] = iter + 1;
        state[ST_RELOC] += moved;
        if (changed == 0) { state[ST_STRICT] = 1; state[ST_DONE] = 1; }
        else if (sh <= tol_abs || iter + 1 >= max_iter) state[ST_DONE] = 1;
    }
}

__global__ __launch_bounds__(256) void km_reset_kernel(int* __restrict__ labels2, int n, int* __restrict__ state) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) labels2[(size_t)n + i] = -1;      // iteration 0 compares with the odd buffer
    if (i < PRAM_KMEANS_STATE_WORDS) state[i] = 0;
}

// ---------------------------------------------------------------------------------------------------------------- blocked sums
// v [n] -> one partial per block: the block through LDS, thread 0 adds it in index order
__global__ __launch_bounds__(256) void km_block_total_kernel(const double* __restrict__ v, int n, double* __restrict__ partial) {
    __shared__ double sv[KB];
    const int tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * KB;
    const int m = n - i0 < KB ? (int)(n - i0) : KB;
    for (int j = tid; j < m; j += 256) sv[j] = v[i0 + j];
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
#pragma unroll 8
        for (int j = 0; j < m; ++j) a += sv[j];
        partial[blockIdx.x] = a;
    }
}

// the partials in block order; one workgroup, through LDS
__global__ __launch_bounds__(256) void km_total_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
    __shared__ double sv[KB];
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int b0 = 0; b0 < nb; b0 += KB) {
        const int m = nb - b0 < KB ? nb - b0 : KB;
        __syncthreads();
        for (int j = tid; j < m; j += 256) sv[j] = partial[b0 + j];
        __syncthreads();
        if (tid == 0) {
#pragma unroll 8
            for (int j = 0; j < m; ++j) a += sv[j];
        }
    }
    if (tid == 0) out[0] = a;
}

// ---------------------------------------------------------------------------------------------------------------- k-means++
// closest [n]; tot [TMAX][nb]: every candidate's potential per block; run [TMAX][nb + 1]: their running sums over the blocks;
// tv / blk / cand [TMAX]: a step's targets, the blocks they fall into and the candidates found; pot[0]: the current potential;
// win[0]: the row of run that belongs to the last winner, win[1]: the winner itself
struct PP { double* closest; double* tot; double* run; double* tv; double* pot; int* cand; int* blk; int* win; };

__global__ __launch_bounds__(256) void km_pp_begin_kernel(int n, int first, PP pp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) pp.closest[i] = pos_inf();
    if (i == 0) { pp.cand[0] = first; pp.win[0] = 0; pp.win[1] = first; }
}

// the potential of candidates 0 .. ntr - 1 inside every block: sum of min(closest, d2(x, x_cand)) in index order
__global__ __launch_bounds__(256) void km_pp_trials_kernel(const double* __restrict__ x, int n, int nb, int ntr, PP pp) {
    __shared__ double sv[TMAX][ROW];
    __shared__ double sx[TMAX][3];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (tid < ntr) {
        int c = pp.cand[tid];
        c = c < 0 ? 0 : (c >= n ? n - 1 : c);
        sx[tid][0] = x[(size_t)c * 3]; sx[tid][1] = x[(size_t)c * 3 + 1]; sx[tid][2] = x[(size_t)c * 3 + 2];
    }
    __syncthreads();
    double acc = 0.0;
    for (int sub = 0; sub < KB / SUB; ++sub) {
        const long long i0 = (long long)b * KB + sub * SUB;
        if (i0 >= n) break;      // uniform
        const long long i = i0 + tid;
        if (i < n) {
            const double x0 = x[i * 3], x1 = x[i * 3 + 1], x2 = x[i * 3 + 2], cl = pp.closest[i];
            for (int t = 0; t < ntr; ++t) {
                const double d = dist2(x0, x1, x2, sx[t][0], sx[t][1], sx[t][2]);
                sv[t][tid] = d < cl ? d : cl;
            }
        }
        __syncthreads();
        const int m = n - i0 < SUB ? (int)(n - i0) : SUB;
        if (tid < ntr) {
#pragma unroll 8
            for (int j = 0; j < m; ++j) acc += sv[tid][j];
        }
        __syncthreads();
    }
    if (tid < ntr) pp.tot[(size_t)tid * nb + b] = acc;
}

// One workgroup: every candidate's running sum over the blocks; the smallest potential wins (the lowest index on a tie) and
// becomes seed `slot`; then for each of the next step's ntr_next targets rand[t] * pot the first block whose running sum reaches
// it.  A target beyond the total leaves blk -1 and the candidate at n - 1 (numpy's clip).
__global__ __launch_bounds__(256) void km_pp_select_kernel(int n, int nb, int ntr_prev, int ntr_next, const double* __restrict__ rand,
                                                           int* __restrict__ seeds, int slot, PP pp) {
    __shared__ double sv[TMAX][ROW];
    __shared__ double pots[TMAX];
    __shared__ int s_win;
    const int tid = threadIdx.x;
    double acc = 0.0;
    if (tid < ntr_prev) pp.run[(size_t)tid * (nb + 1)] = 0.0;
    for (int b0 = 0; b0 < nb; b0 += SUB) {
        const int m = nb - b0 < SUB ? nb - b0 : SUB;
        __syncthreads();
        if (tid < m)
            for (int t = 0; t < ntr_prev; ++t) sv[t][tid] = pp.tot[(size_t)t * nb + b0 + tid];
        __syncthreads();
        if (tid < ntr_prev) {
#pragma unroll 8
            for (int j = 0; j < m; ++j) {
                acc += sv[tid][j];
                pp.run[(size_t)tid * (nb + 1) + b0 + j + 1] = acc;
            }
        }
    }
    if (tid < ntr_prev) pots[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        int w = 0;
        for (int t = 1; t < ntr_prev; ++t)
            if (pots[t] < pots[w]) w = t;
        int c = pp.cand[w];
        c = c < 0 ? 0 : (c >= n ? n - 1 : c);
        s_win = w;
        pp.win[0] = w;
        pp.win[1] = c;
        seeds[slot] = c;
        pp.pot[0] = pots[w];
    }
    __syncthreads();      // the winner's run and the old candidates are read, the new ones written below
    if (tid < ntr_next) {
        const double v = rand[tid] * pots[s_win];
        const double* __restrict__ r = pp.run + (size_t)s_win * (nb + 1);
        const int lo = first_true(0, nb, [&](int b) { return !(r[b + 1] < v); });      // the first block whose running sum reaches v
        pp.tv[tid] = v;
        pp.blk[tid] = lo < nb ? lo : -1;
        pp.cand[tid] = n - 1;
    }
}

// Every block takes the new seed into closest; a block that a target falls into walks its running sum to the first point that
// reaches the target (thread t walks for target t).
__global__ __launch_bounds__(256) void km_pp_update_kernel(const double* __restrict__ x, int n, int nb, int ntr, PP pp) {
    __shared__ double sv[SUB];
    const int tid = threadIdx.x, b = blockIdx.x;
    int seed = pp.win[1], w = pp.win[0];
    seed = seed < 0 ? 0 : (seed >= n ? n - 1 : seed);
    w = w < 0 ? 0 : (w >= TMAX ? TMAX - 1 : w);
    const double s0 = x[(size_t)seed * 3], s1 = x[(size_t)seed * 3 + 1], s2 = x[(size_t)seed * 3 + 2];
    const bool mine = tid < ntr && pp.blk[tid] == b;
    const double v = mine ? pp.tv[tid] : 0.0, base = mine ? pp.run[(size_t)w * (nb + 1) + b] : 0.0;
    double acc = 0.0;
    long long found = -1;
    for (int sub = 0; sub < KB / SUB; ++sub) {
        const long long i0 = (long long)b * KB + sub * SUB;
        if (i0 >= n) break;      // uniform
        const long long i = i0 + tid;
        if (i < n) {
            const double d = dist2(x[i * 3], x[i * 3 + 1], x[i * 3 + 2], s0, s1, s2), cl = pp.closest[i];
            const double m2 = d < cl ? d : cl;
            pp.closest[i] = m2;
            sv[tid] = m2;
        }
        __syncthreads();
        const int m = n - i0 < SUB ? (int)(n - i0) : SUB;
        if (mine && found < 0) {
            for (int j = 0; j < m; ++j) {
                acc += sv[j];
                if (base + acc >= v) { found = i0 + j; break; }
            }
        }
        __syncthreads();
    }
    if (mine && found >= 0) pp.cand[tid] = (int)found;
}

__global__ __launch_bounds__(256) void km_gather_kernel(const double* __restrict__ x, int n, const int* __restrict__ seeds, int k,
                                                        double* __restrict__ centers) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    int s = seeds[c];
    s = s < 0 ? 0 : (s >= n ? n - 1 : s);
    centers[(size_t)c * 3] = x[(size_t)s * 3]; centers[(size_t)c * 3 + 1] = x[(size_t)s * 3 + 1]; centers[(size_t)c * 3 + 2] = x[(size_t)s * 3 + 2];
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct Layout {
    size_t part, sums, ipart, closest, tot, run, tv, pot;      // float64 segments, in doubles from the start
    size_t labels2, cnt, counts, empties, cand, blk, win;      // int32 segments, in ints from the end of the doubles
    size_t n_doubles, n_ints;
};

static Layout layout(long long n, int k) {
    const size_t nb = (size_t)((n + KB - 1) / KB), N = (size_t)n, K = (size_t)k;
    Layout L;
    size_t d = 0, i = 0;
    L.part = d; d += nb * 3 * K;
    L.sums = d; d += 3 * K;
    L.ipart = d; d += nb;
    L.closest = d; d += N;
    L.tot = d; d += (size_t)TMAX * nb;
    L.run = d; d += (size_t)TMAX * (nb + 1);
    L.tv = d; d += TMAX;
    L.pot = d; d += 2;
    L.labels2 = i; i += 2 * N;
    L.cnt = i; i += nb * K;
    L.counts = i; i += K;
    L.empties = i; i += K;
    L.cand = i; i += TMAX;
    L.blk = i; i += TMAX;
    L.win = i; i += 2;
    L.n_doubles = d;
    L.n_ints = i;
    return L;
}

static bool shape_ok(long long n, int k) { return n >= 1 && n < (1LL << 31) && k >= 1 && k <= n && k <= KMAX; }

#define KM_SHAPE(what)                                                                                                                 \
    PRAM_REQUIRE(shape_ok(n, k), what ": needs 1 <= n < 2^31 and 1 <= k <= min(n, %d), got n = %lld, k = %d", KMAX, n, k)

}  // namespace

extern "C" size_t pram_kmeans_workspace_bytes(long long n, int k) {
    if (!shape_ok(n, k)) return 0;
    const Layout L = layout(n, k);
    return 8 * L.n_doubles + 4 * L.n_ints;
}

extern "C" int pram_kmeans_init_pp(const double* x, long long n, int k, int first, const double* rand, int n_trials, void* workspace,
                                   size_t workspace_bytes, int* seeds, double* centers, void* stream) {
    PRAM_REQUIRE(x && workspace && seeds && centers && (rand || k == 1), "pram_kmeans_init_pp: null pointer");
    PRAM_REQUIRE(aligned(x, 8) && aligned(rand, 8) && aligned(workspace, 8) && aligned(centers, 8), "pram_kmeans_init_pp: float64 buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(seeds, 4), "pram_kmeans_init_pp: misaligned pointer");
    KM_SHAPE("pram_kmeans_init_pp");
    PRAM_REQUIRE(first >= 0 && first < n, "pram_kmeans_init_pp: the first seed %d is no point", first);
    PRAM_REQUIRE(n_trials >= 1 && n_trials <= TMAX, "pram_kmeans_init_pp: needs 1 <= n_trials <= %d", TMAX);
    const Layout L = layout(n, k);
    const size_t need = 8 * L.n_doubles + 4 * L.n_ints;
    PRAM_REQUIRE(workspace_bytes >= need, "pram_kmeans_init_pp: workspace of %zu bytes, needs %zu (pram_kmeans_workspace_bytes)", workspace_bytes, need);
    double* wd = static_cast<double*>(workspace);
    int* wi = reinterpret_cast<int*>(wd + L.n_doubles);
    PP pp = {wd + L.closest, wd + L.tot, wd + L.run, wd + L.tv, wd + L.pot, wi + L.cand, wi + L.blk, wi + L.win};
    const int N = (int)n, nb = (int)((n + KB - 1) / KB);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(km_pp_begin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, N, first, pp);
    hipLaunchKernelGGL(km_pp_trials_kernel, dim3(nb), dim3(256), 0, s, x, N, nb, 1, pp);
    for (int c = 1; c < k; ++c) {
        hipLaunchKernelGGL(km_pp_select_kernel, dim3(1), dim3(256), 0, s, N, nb, c == 1 ? 1 : n_trials, n_trials, rand + (size_t)(c - 1) * n_trials, seeds,
                           c - 1, pp);
        hipLaunchKernelGGL(km_pp_update_kernel, dim3(nb), dim3(256), 0, s, x, N, nb, n_trials, pp);
        hipLaunchKernelGGL(km_pp_trials_kernel, dim3(nb), dim3(256), 0, s, x, N, nb, n_trials, pp);
    }
    hipLaunchKernelGGL(km_pp_select_kernel, dim3(1), dim3(256), 0, s, N, nb, k == 1 ? 1 : n_trials, 0, rand, seeds, k - 1, pp);
    hipLaunchKernelGGL(km_gather_kernel, dim3((k + 255) / 256), dim3(256), 0, s, x, N, seeds, k, centers);
    return pram_launch_status("pram_kmeans_init_pp");
}

extern "C" int pram_kmeans_lloyd(const double* x, long long n, int k, double* centers, double tol_abs, int max_iter, int first_iter, int n_iters,
                                 int finish, void* workspace, size_t workspace_bytes, int* labels, double* dist, int* state, double* inertia,
                                 void* stream) {
    PRAM_REQUIRE(x && centers && workspace && labels && dist && state && inertia, "pram_kmeans_lloyd: null pointer");
    PRAM_REQUIRE(aligned(x, 8) && aligned(centers, 8) && aligned(workspace, 8) && aligned(dist, 8) && aligned(inertia, 8),
                 "pram_kmeans_lloyd: float64 buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(labels, 4) && aligned(state, 4), "pram_kmeans_lloyd: misaligned pointer");
    KM_SHAPE("pram_kmeans_lloyd");
    PRAM_REQUIRE(max_iter >= 1 && first_iter >= 0 && n_iters >= 0 && first_iter <= max_iter && n_iters <= max_iter - first_iter,
                 "pram_kmeans_lloyd: needs max_iter >= 1 and iterations first_iter .. first_iter + n_iters inside [0, max_iter]");
    PRAM_REQUIRE(tol_abs >= 0.0, "pram_kmeans_lloyd: needs tol_abs >= 0");
    const Layout L = layout(n, k);
    const size_t need = 8 * L.n_doubles + 4 * L.n_ints;
    PRAM_REQUIRE(workspace_bytes >= need, "pram_kmeans_lloyd: workspace of %zu bytes, needs %zu (pram_kmeans_workspace_bytes)", workspace_bytes, need);
    double* wd = static_cast<double*>(workspace);
    int* wi = reinterpret_cast<int*>(wd + L.n_doubles);
    double *part = wd + L.part, *sums = wd + L.sums, *ipart = wd + L.ipart;
    int *labels2 = wi + L.labels2, *cnt = wi + L.cnt, *counts = wi + L.counts, *empties = wi + L.empties;
    const int N = (int)n, nb = (int)((n + KB - 1) / KB);
    const unsigned pgrid = (unsigned)((n + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (first_iter == 0) hipLaunchKernelGGL(km_reset_kernel, dim3(pgrid), dim3(256), 0, s, labels2, N, state);
    for (int it = first_iter; it < first_iter + n_iters; ++it) {
        hipLaunchKernelGGL(km_assign_kernel<1>, dim3(pgrid), dim3(256), 0, s, x, N, centers, k, (int*)nullptr, dist, labels2, it, state);
        hipLaunchKernelGGL(km_block_sums_kernel, dim3(nb), dim3(KB), 0, s, x, N, k, labels2, it, part, cnt, state);
        hipLaunchKernelGGL(km_reduce_kernel, dim3((4 * k + 255) / 256), dim3(256), 0, s, part, cnt, nb, k, sums, counts, state);
        hipLaunchKernelGGL(km_update_kernel, dim3(1), dim3(256), 0, s, x, N, k, centers, sums, counts, labels2, dist, empties, state, inertia + 1, tol_abs,
                           max_iter, it);
    }
    if (finish != 0) {
        hipLaunchKernelGGL(km_assign_kernel<2>, dim3(pgrid), dim3(256), 0, s, x, N, centers, k, labels, dist, labels2, 0, state);
        hipLaunchKernelGGL(km_block_total_kernel, dim3(nb), dim3(256), 0, s, dist, N, ipart);
        hipLaunchKernelGGL(km_total_kernel, dim3(1), dim3(256), 0, s, ipart, nb, inertia);
    }
    return pram_launch_status("pram_kmeans_lloyd");
}

extern "C" int pram_kmeans_assign(const double* x, long long n, const double* centers, int k, int* labels, double* dist, void* stream) {
    PRAM_REQUIRE(x && centers && labels && dist, "pram_kmeans_assign: null pointer");
    PRAM_REQUIRE(aligned(x, 8) && aligned(centers, 8) && aligned(dist, 8), "pram_kmeans_assign: float64 buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(labels, 4), "pram_kmeans_assign: misaligned pointer");
    KM_SHAPE("pram_kmeans_assign");
    hipLaunchKernelGGL(km_assign_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (int)n, centers, k, labels, dist,
                       (int*)nullptr, 0, (int*)nullptr);
    return pram_launch_status("pram_kmeans_assign");
}
