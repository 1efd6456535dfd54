// Map compression: RecMap.compress_map_by_projection_v2 of the reference (recognition/recmap.py:668-922) and the projection that
// RefFrame.associate_keypoints_with_point3Ds (localization/refframe.py:99-147) puts in place of a compressed frame's keypoints.
//   * selection (recmap.py:695-828): the frames are taken in the order of the virtual reference frames and their covisible lists.
//     A frame that is not retained yet keeps the rows that no frame of the current chain already covers: a row is dropped when it
//     projects into a chain frame, in front of it, within `radius` pixels of one of that frame's kept keypoints.  The state
//     (retained order, kept flag per row, the chain) lives on the device; the host enqueues a begin step per reference frame and
//     a test and a commit step per candidate, and reads nothing back in between.  The kernels decide from the state whether a
//     step appends, tests or does nothing.  No workgroup waits for another.
//   * sparsification (recmap.py:670-693, 852-860): one workgroup per frame, the best point of every grid cell.
//   * rows of the compressed frames: gather and projection per listed point.
// Float64 throughout, every product and sum written out (the library is built with -ffp-contract=off); plain stores only, every
// one of them idempotent or owned by one thread; every index read from a table is checked against the size given beside it.
#include "glue.h"

namespace {

constexpr int CP_ROWS = PRAM_COMPRESS_ROW_TILE;
constexpr int CP_KPTS = PRAM_COMPRESS_KPT_TILE;
constexpr int CP_GROUP = 8;      // keypoints of a tile measured between two looks at the result
static_assert(CP_ROWS == 256 && CP_KPTS == 256, "one row and one staged keypoint per thread of a 256-thread workgroup");
static_assert(CP_KPTS % CP_GROUP == 0, "a tile is a whole number of groups");

struct Cam { double r00, r01, r02, r10, r11, r12, r20, r21, r22, tx, ty, tz, fx, fy, cx, cy, w, h; };

__device__ __forceinline__ Cam load_cam(const double* __restrict__ cam) {
    const double qw = cam[0], qx = cam[1], qy = cam[2], qz = cam[3];
    Cam c;
    c.r00 = 1.0 - 2.0 * qy * qy - 2.0 * qz * qz; c.r01 = 2.0 * qx * qy - 2.0 * qw * qz; c.r02 = 2.0 * qz * qx + 2.0 * qw * qy;
    c.r10 = 2.0 * qx * qy + 2.0 * qw * qz; c.r11 = 1.0 - 2.0 * qx * qx - 2.0 * qz * qz; c.r12 = 2.0 * qy * qz - 2.0 * qw * qx;
    c.r20 = 2.0 * qz * qx - 2.0 * qw * qy; c.r21 = 2.0 * qy * qz + 2.0 * qw * qx; c.r22 = 1.0 - 2.0 * qx * qx - 2.0 * qy * qy;
    c.tx = cam[4]; c.ty = cam[5]; c.tz = cam[6];
    c.fx = cam[7]; c.fy = cam[8]; c.cx = cam[9]; c.cy = cam[10]; c.w = cam[11]; c.h = cam[12];
    return c;
}

// p = R x + t, u = (fx p_x + cx p_z) / p_z, v likewise: the reference's K (T x) with the products added left to right
__device__ __forceinline__ void project(const Cam& c, double x, double y, double z, double& u, double& v, double& Z) {
    const double X = c.r00 * x + c.r01 * y + c.r02 * z + c.tx, Y = c.r10 * x + c.r11 * y + c.r12 * z + c.ty;
    Z = c.r20 * x + c.r21 * y + c.r22 * z + c.tz;
    u = (c.fx * X + c.cx * Z) / Z;
    v = (c.fy * Y + c.cy * Z) / Z;
}

// the device state of one selection: all of it in the caller's workspace
struct SelState { int* row_pt; int* kept; int* disc; int* chain; int* counts; };      // counts[0]: chain length, counts[1]: frames retained

// Frame f's rows, cut by hand and not by glue.h's clamped_range: the callers iterate [r0, r1) or cap a count at r1 - r0 that is
// compared with nkpts >= 1, so the two agree, but clamped_range's two further bounds measured 1.3 % on pram_compress_select, whose
// thousands of one-workgroup launches are each a few instructions long (profiles/geometry_shared_code.md).
__device__ __forceinline__ void frame_rows(const int* __restrict__ frame_off, int f, int n_rows, int& r0, int& r1) {
    r0 = frame_off[f];
    r1 = frame_off[f + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > n_rows ? n_rows : r1;
}

// every row's index in the point table (-1: id -1 or an id the table lacks: not a valid row), nothing kept, nothing retained
__global__ __launch_bounds__(256) void compress_init_kernel(const long long* __restrict__ ids, int n_rows, const long long* __restrict__ pt_ids,
                                                            int n_points, int n_frames, int cap, SelState st, int* __restrict__ ret_order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_rows) {
        const long long id = ids[i];
        int p = -1;
        if (id != -1) {
            const int lo = lower_bound_i64(pt_ids, n_points, id);
            if (lo < n_points && pt_ids[lo] == id) p = lo;
        }
        st.row_pt[i] = p;
        st.kept[i] = 0;
        st.disc[i] = -1;
    }
    if (i < n_frames) ret_order[i] = -1;
    if (i < cap) st.chain[i] = -1;
    if (i < 2) st.counts[i] = 0;
}

// recmap.py:771-805: the reference frame v is retained with all its valid rows (over an earlier partial retention, keeping its
// place in the retained order) and starts the chain.  One workgroup.
__global__ __launch_bounds__(256) void compress_begin_kernel(const int* __restrict__ frame_off, int n_rows, int v, SelState st,
                                                             int* __restrict__ ret_order) {
    int r0, r1;
    frame_rows(frame_off, v, n_rows, r0, r1);
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) st.kept[r] = st.row_pt[r] >= 0;
    if (threadIdx.x == 0) {
        if (ret_order[v] < 0) ret_order[v] = st.counts[1]++;
        st.chain[0] = v;
        st.counts[0] = 1;
    }
}

// choose_valid_p3ds (recmap.py:695-747) for candidate c: workgroup (x, y) tests the rows x * CP_ROWS .. of c against chain slot y.
// A retained candidate and an empty slot are nothing to do.  A row found within the radius writes the step's number over its
// discard word: several workgroups may write the same value, nobody reads it before the commit.
__global__ __launch_bounds__(256) void compress_test_kernel(const int* __restrict__ frame_off, int n_frames, int n_rows,
                                                            const double* __restrict__ pt_xyz, const double* __restrict__ xys,
                                                            const double* __restrict__ cams, int c, int step, int cap, double radius,
                                                            double r2_lo, double r2_hi, SelState st, const int* __restrict__ ret_order) {
    __shared__ double2 s_xy[CP_KPTS];
    const int tid = threadIdx.x, slot = blockIdx.y;
    if (ret_order[c] >= 0) return;
    int n_chain = st.counts[0];
    n_chain = n_chain > cap ? cap : n_chain;
    if (slot >= n_chain) return;
    const int kf = st.chain[slot];
    if (kf < 0 || kf >= n_frames) return;
    int r0, r1, k0, k1;
    frame_rows(frame_off, c, n_rows, r0, r1);
    frame_rows(frame_off, kf, n_rows, k0, k1);
    const int r = r0 + blockIdx.x * CP_ROWS + tid;
    const int p = r < r1 ? st.row_pt[r] : -1;
    bool live = false;
    double u = 0.0, v = 0.0;
    if (p >= 0) {
        const Cam cam = load_cam(cams + (size_t)kf * PRAM_MAPBUILD_CAM_COLS);
        double Z;
        project(cam, pt_xyz[(size_t)p * 3], pt_xyz[(size_t)p * 3 + 1], pt_xyz[(size_t)p * 3 + 2], u, v, Z);
        live = u >= 0.0 && u < cam.w && v >= 0.0 && v < cam.h && Z > 0.0;
    }
    bool found = false;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int j0 = k0; j0 < k1; j0 += CP_KPTS) {
        // also the barrier between the previous tile's readers and this tile's writers; uniform: leaves when no row is left to decide
        if (!__syncthreads_or(live && !found)) break;
        const int j = j0 + tid;
        // a keypoint that is not kept, and a slot past the frame's last row, lies nowhere: NaN compares false
        const bool on = j < k1 && st.kept[j] != 0;
        s_xy[tid] = on ? make_double2(xys[(size_t)j * 2], xys[(size_t)j * 2 + 1]) : make_double2(nan, nan);
        __syncthreads();
        if (live && !found) {
            // sqrt(d2) <= radius is the reference's test; d2 outside [r2_lo, r2_hi] decides it without the root.  Eight keypoints
            // at a time without a branch between them (a row's walk is one lane's chain of LDS reads); the root only for a group
            // with a keypoint inside the band and none below it.
            for (int t = 0; t < CP_KPTS && !found; t += CP_GROUP) {
                bool below = false, band = false;
#pragma unroll
                for (int q = 0; q < CP_GROUP; ++q) {
                    const double2 k = s_xy[t + q];
                    const double dx = u - k.x, dy = v - k.y;
                    const double d2 = dx * dx + dy * dy;
                    below |= d2 <= r2_lo;
                    band |= d2 <= r2_hi;
                }
                found = below;
                if (!below && band) {
                    for (int q = 0; q < CP_GROUP; ++q) {
                        const double2 k = s_xy[t + q];
                        const double dx = u - k.x, dy = v - k.y;
                        const double d2 = dx * dx + dy * dy;
                        found |= d2 <= r2_hi && sqrt(d2) <= radius;
                    }
                }
            }
        }
    }
    if (found) st.disc[r] = step;
}

// recmap.py:806-828 after the test: a retained candidate joins the chain; one that was tested keeps the rows no chain frame
// covered and, with at least one left, is retained and joins the chain.  One workgroup.
__global__ __launch_bounds__(256) void compress_commit_kernel(const int* __restrict__ frame_off, int n_rows, int c, int step, int cap,
                                                              SelState st, int* __restrict__ ret_order) {
    __shared__ int s4[4];
    const int tid = threadIdx.x;
    const bool was = ret_order[c] >= 0;
    int n = 0;
    if (!was) {
        int r0, r1;
        frame_rows(frame_off, c, n_rows, r0, r1);
        for (int r = r0 + tid; r < r1; r += 256) {
            const int keep = st.row_pt[r] >= 0 && st.disc[r] != step;
            st.kept[r] = keep;
            n += keep;
        }
    }
    n = wave_sum_i32(n);
    if ((tid & 63) == 0) s4[tid >> 6] = n;
    __syncthreads();      // not block_sum_i32: s4 is written once and thread 0 alone reads the sum, so one barrier does
    if (tid == 0 && (was || s4[0] + s4[1] + s4[2] + s4[3] > 0)) {
        if (!was) ret_order[c] = st.counts[1]++;
        const int len = st.counts[0];
        if (len < cap) { st.chain[len] = c; st.counts[0] = len + 1; }
    }
}

// the kept rows of every frame as point table indices, in row order, packed to the front of the frame's own range
__global__ __launch_bounds__(256) void compress_lists_kernel(const int* __restrict__ frame_off, int n_rows, SelState st,
                                                             const int* __restrict__ ret_order, int* __restrict__ list_pt,
                                                             int* __restrict__ list_cnt) {
    __shared__ int wsum[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    int r0, r1, base = 0;
    frame_rows(frame_off, f, n_rows, r0, r1);
    if (ret_order[f] < 0) r1 = r0;
    for (int q0 = r0; q0 < r1; q0 += 256) {
        const int r = q0 + tid;
        const bool keep = r < r1 && st.kept[r] != 0;
        int total;
        const int o = chunk_offset<4>(keep, wsum, total);
        if (keep) list_pt[r0 + base + o] = st.row_pt[r];
        base += total;
    }
    if (tid == 0) list_cnt[f] = base;
}

// numpy's float floor division a // b for b > 0 (npy_divmod: fmod first, then the quotient of the difference)
__device__ __forceinline__ double np_floor_divide(double a, double b) {
    const double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0 && mod < 0.0) div -= 1.0;
    if (div != 0.0) {
        double fl = floor(div);
        if (div - fl > 0.5) fl += 1.0;
        return fl;
    }
    return copysign(0.0, a / b);
}

struct SparseWs { unsigned long long* key; int* score; int* first; int* rank; int* out; };

// sparsify_by_grid (recmap.py:670-693) on every frame that lists more than nkpts points.  One workgroup per frame; position i of
// the list is its key (the grid cell of its projection) and its score.  The winner of a cell is the first position with the
// cell's highest score; winners leave in the order in which their cells first appear.  A position whose projection is not finite
// (or whose cell no 64-bit integer holds) takes no part.
__global__ __launch_bounds__(256) void compress_sparsify_kernel(const int* __restrict__ frame_off, int n_rows, const double* __restrict__ cams,
                                                                const double* __restrict__ pt_xyz, const int* __restrict__ pt_score,
                                                                int n_points, double radius, int nkpts, SparseWs ws,
                                                                int* __restrict__ list_pt, int* __restrict__ list_cnt) {
    __shared__ int wsum[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    int r0, r1;
    frame_rows(frame_off, f, n_rows, r0, r1);
    int n = list_cnt[f];
    n = n > r1 - r0 ? r1 - r0 : n;
    if (n <= nkpts) return;
    const Cam cam = load_cam(cams + (size_t)f * PRAM_MAPBUILD_CAM_COLS);
    const double nw_d = ceil(cam.w / radius);
    const unsigned long long nw = fabs(nw_d) < 4.0e18 ? (unsigned long long)(long long)nw_d : 0ull;
    unsigned long long* key = ws.key + r0;
    int *score = ws.score + r0, *first = ws.first + r0, *rank = ws.rank + r0, *out = ws.out + r0, *list = list_pt + r0;
    for (int i = tid; i < n; i += 256) {
        const int p = list[i];
        int s = -1;
        unsigned long long k = 0ull;
        if (p >= 0 && p < n_points) {
            double u, v, Z;
            project(cam, pt_xyz[(size_t)p * 3], pt_xyz[(size_t)p * 3 + 1], pt_xyz[(size_t)p * 3 + 2], u, v, Z);
            if (isfinite(u) && isfinite(v)) {
                const double iw = rint(np_floor_divide(u, radius)), ih = rint(np_floor_divide(v, radius));
                if (fabs(iw) < 4.0e18 && fabs(ih) < 4.0e18) {
                    k = (unsigned long long)(long long)ih * nw + (unsigned long long)(long long)iw;      // wraps as int64 does
                    s = pt_score[p] < 0 ? 0 : pt_score[p];
                }
            }
        }
        key[i] = k;
        score[i] = s;
    }
    __syncthreads();
    // first[i]: the first position of i's cell when i is its winner, -1 otherwise; rank[i] = 1 for the first position of a cell
    for (int i = tid; i < n; i += 256) {
        const unsigned long long k = key[i];
        const int s = score[i];
        int fi = -1;
        bool beaten = s < 0;
        for (int j = 0; j < n && s >= 0; ++j) {
            const int sj = score[j];
            if (sj < 0 || key[j] != k) continue;
            if (fi < 0) fi = j;
            beaten |= sj > s || (sj == s && j < i);
        }
        first[i] = beaten ? -1 : fi;
        rank[i] = fi == i;
    }
    __syncthreads();
    // rank[j] -> the number of cells that appear before position j
    int base = 0;
    for (int q0 = 0; q0 < n; q0 += 256) {
        const int j = q0 + tid;
        const bool is_first = j < n && rank[j] != 0;
        int total;
        const int o = chunk_offset<4>(is_first, wsum, total);
        if (j < n) rank[j] = base + o;
        base += total;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256)
        if (first[i] >= 0) out[rank[first[i]]] = list[i];
    __syncthreads();
    for (int i = tid; i < base; i += 256) list[i] = out[i];
    if (tid == 0) list_cnt[f] = base;
}

// associate_keypoints_with_point3Ds (refframe.py:99-147): row i of the compressed map is point row_point[i] seen from frame
// row_frame[i].  Half a wave per row: 32 lanes copy the descriptor, the first one projects.
__global__ __launch_bounds__(256) void compress_rows_kernel(const int* __restrict__ row_frame, const int* __restrict__ row_point, int n_out,
                                                            int n_frames, int n_points, const double* __restrict__ cams,
                                                            const long long* __restrict__ pt_ids, const double* __restrict__ pt_xyz,
                                                            const float4* __restrict__ pt_desc, const int* __restrict__ pt_sid,
                                                            const double* __restrict__ pt_err, double* __restrict__ out_kpts,
                                                            double* __restrict__ out_xyz, float4* __restrict__ out_desc,
                                                            int* __restrict__ out_sid, long long* __restrict__ out_ids) {
    const int i = blockIdx.x * 8 + (threadIdx.x >> 5), q = threadIdx.x & 31;
    if (i >= n_out) return;
    const int f = row_frame[i], p = row_point[i];
    const bool ok = f >= 0 && f < n_frames && p >= 0 && p < n_points;
    out_desc[(size_t)i * 32 + q] = ok ? pt_desc[(size_t)p * 32 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (q != 0) return;
    double x = 0.0, y = 0.0, z = 0.0, u = 0.0, v = 0.0, s = 0.0;
    if (ok) {
        const Cam cam = load_cam(cams + (size_t)f * PRAM_MAPBUILD_CAM_COLS);
        x = pt_xyz[(size_t)p * 3]; y = pt_xyz[(size_t)p * 3 + 1]; z = pt_xyz[(size_t)p * 3 + 2];
        double Z;
        project(cam, x, y, z, u, v, Z);
        double e = pt_err[p] * 5.0;      // 1 / clip(5 error, 1, 20); np.clip hands a NaN through
        e = e < 1.0 ? 1.0 : (e > 20.0 ? 20.0 : e);
        s = 1.0 / e;
    }
    out_kpts[(size_t)i * 3] = u; out_kpts[(size_t)i * 3 + 1] = v; out_kpts[(size_t)i * 3 + 2] = s;
    out_xyz[(size_t)i * 3] = x; out_xyz[(size_t)i * 3 + 1] = y; out_xyz[(size_t)i * 3 + 2] = z;
    out_sid[i] = ok ? pt_sid[p] : -1;
    out_ids[i] = ok ? pt_ids[p] : -1;
}

static bool offsets_ok(const int* off, int n) {
    if (off[0] != 0) return false;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// the workspace serves the selection (three words per row, the chain, two counters) and the sparsification (six words per row)
static size_t ws_bytes(int n_rows, int covisibility_frame) { return 24 * (size_t)n_rows + 4 * ((size_t)covisibility_frame + 1) + 16; }

}  // namespace

extern "C" size_t pram_compress_workspace_bytes(int n_rows, int covisibility_frame) {
    if (n_rows < 0 || covisibility_frame < 0) return 0;
    return ws_bytes(n_rows, covisibility_frame);
}

extern "C" int pram_compress_select(const long long* point3d_ids, const int* frame_off, const int* frame_off_host, int n_frames, int n_rows,
                                    const long long* pt_ids, int n_points, const double* pt_xyz, const double* xys, const double* frame_cams,
                                    const int* covis_off_host, const int* covis_frames_host, int covisibility_frame, const int* vrf_host,
                                    int n_vrf, double radius, void* workspace, size_t workspace_bytes, int* ret_order, int* list_cnt,
                                    int* list_pt, void* stream) {
    PRAM_REQUIRE(point3d_ids && frame_off && frame_off_host && pt_ids && pt_xyz && xys && frame_cams && covis_off_host && covis_frames_host &&
                 vrf_host && workspace && ret_order && list_cnt && list_pt, "pram_compress_select: null pointer");
    PRAM_REQUIRE(aligned(point3d_ids, 8) && aligned(pt_ids, 8) && aligned(pt_xyz, 8) && aligned(xys, 8) && aligned(frame_cams, 8) &&
                 aligned(workspace, 8), "pram_compress_select: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(frame_off, 4) && aligned(ret_order, 4) && aligned(list_cnt, 4) && aligned(list_pt, 4), "pram_compress_select: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 1 && n_rows >= 0 && n_points >= 0 && n_vrf >= 0 && covisibility_frame >= 1,
                 "pram_compress_select: needs n_frames >= 1, n_rows >= 0, n_points >= 0, n_vrf >= 0, covisibility_frame >= 1");
    PRAM_REQUIRE((radius == 0.0 || radius > 1e-150) && radius < 1e150, "pram_compress_select: needs a finite radius >= 0");
    PRAM_REQUIRE(offsets_ok(frame_off_host, n_frames) && frame_off_host[n_frames] == n_rows,
                 "pram_compress_select: frame_off must start at 0, not decrease and end at n_rows");
    PRAM_REQUIRE(offsets_ok(covis_off_host, n_frames), "pram_compress_select: covis_off must start at 0 and not decrease");
    for (int i = 0; i < covis_off_host[n_frames]; ++i)
        PRAM_REQUIRE(covis_frames_host[i] >= 0 && covis_frames_host[i] < n_frames, "pram_compress_select: covis_frames[%d] = %d is no frame", i,
                     covis_frames_host[i]);
    for (int i = 0; i < n_vrf; ++i) {
        const int v = vrf_host[i];
        PRAM_REQUIRE(v >= 0 && v < n_frames, "pram_compress_select: reference frame %d is no frame", v);
        const int len = covis_off_host[v + 1] - covis_off_host[v];
        PRAM_REQUIRE(len >= 1, "pram_compress_select: reference frame %d has no covisible list (a store built with it among seg_ref_frame_ids has)", v);
        PRAM_REQUIRE(len <= covisibility_frame, "pram_compress_select: the covisible list of frame %d has %d entries, covisibility_frame is %d", v, len,
                     covisibility_frame);
    }
    const size_t need = ws_bytes(n_rows, covisibility_frame);
    PRAM_REQUIRE(workspace_bytes >= need, "pram_compress_select: workspace of %zu bytes, needs %zu (pram_compress_workspace_bytes)", workspace_bytes, need);
    const int cap = covisibility_frame + 1;
    SelState st;
    st.row_pt = static_cast<int*>(workspace);
    st.kept = st.row_pt + n_rows;
    st.disc = st.kept + n_rows;
    st.chain = st.disc + n_rows;
    st.counts = st.chain + cap;
    hipStream_t s = (hipStream_t)stream;
    const int most = n_rows > n_frames ? (n_rows > cap ? n_rows : cap) : (n_frames > cap ? n_frames : cap);
    hipLaunchKernelGGL(compress_init_kernel, dim3((most + 255) / 256), dim3(256), 0, s, point3d_ids, n_rows, pt_ids, n_points, n_frames, cap, st, ret_order);
    const double r2 = radius * radius, r2_lo = r2 * (1.0 - 1e-12), r2_hi = r2 * (1.0 + 1e-12);
    int step = 0;
    for (int i = 0; i < n_vrf; ++i) {
        const int v = vrf_host[i];
        hipLaunchKernelGGL(compress_begin_kernel, dim3(1), dim3(256), 0, s, frame_off, n_rows, v, st, ret_order);
        for (int e = covis_off_host[v]; e < covis_off_host[v + 1]; ++e) {
            const int c = covis_frames_host[e];
            if (c == v) continue;
            const int rows = frame_off_host[c + 1] - frame_off_host[c];
            if (rows > 0)
                hipLaunchKernelGGL(compress_test_kernel, dim3((rows + CP_ROWS - 1) / CP_ROWS, cap), dim3(256), 0, s, frame_off, n_frames, n_rows, pt_xyz,
                                   xys, frame_cams, c, step, cap, radius, r2_lo, r2_hi, st, ret_order);
            hipLaunchKernelGGL(compress_commit_kernel, dim3(1), dim3(256), 0, s, frame_off, n_rows, c, step, cap, st, ret_order);
            ++step;
        }
    }
    hipLaunchKernelGGL(compress_lists_kernel, dim3(n_frames), dim3(256), 0, s, frame_off, n_rows, st, ret_order, list_pt, list_cnt);
    return pram_launch_status("pram_compress_select");
}

extern "C" int pram_compress_sparsify(const int* frame_off, int n_frames, int n_rows, const double* frame_cams, const double* pt_xyz,
                                      const int* pt_score, int n_points, double radius, int nkpts, void* workspace, size_t workspace_bytes,
                                      int* list_pt, int* list_cnt, void* stream) {
    PRAM_REQUIRE(frame_off && frame_cams && pt_xyz && pt_score && workspace && list_pt && list_cnt, "pram_compress_sparsify: null pointer");
    PRAM_REQUIRE(aligned(frame_cams, 8) && aligned(pt_xyz, 8) && aligned(workspace, 8), "pram_compress_sparsify: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(frame_off, 4) && aligned(pt_score, 4) && aligned(list_pt, 4) && aligned(list_cnt, 4), "pram_compress_sparsify: misaligned pointer");
    PRAM_REQUIRE(n_frames >= 1 && n_rows >= 0 && n_points >= 0 && nkpts >= 1, "pram_compress_sparsify: needs n_frames >= 1, n_rows >= 0, n_points >= 0, nkpts >= 1");
    PRAM_REQUIRE(radius > 0.0 && radius < 1e150, "pram_compress_sparsify: needs a finite radius > 0");
    const size_t need = ws_bytes(n_rows, 0);
    PRAM_REQUIRE(workspace_bytes >= need, "pram_compress_sparsify: workspace of %zu bytes, needs %zu (pram_compress_workspace_bytes)", workspace_bytes, need);
    SparseWs ws;
    ws.key = static_cast<unsigned long long*>(workspace);
    ws.score = reinterpret_cast<int*>(ws.key + n_rows);
    ws.first = ws.score + n_rows;
    ws.rank = ws.first + n_rows;
    ws.out = ws.rank + n_rows;
    hipLaunchKernelGGL(compress_sparsify_kernel, dim3(n_frames), dim3(256), 0, (hipStream_t)stream, frame_off, n_rows, frame_cams, pt_xyz, pt_score,
                       n_points, radius, nkpts, ws, list_pt, list_cnt);
    return pram_launch_status("pram_compress_sparsify");
}

extern "C" int pram_compress_rows(const int* row_frame, const int* row_point, int n_out, int n_frames, int n_points, const double* frame_cams,
                                  const long long* pt_ids, const double* pt_xyz, const float* pt_desc, const int* pt_sid, const double* pt_err,
                                  double* out_kpts, double* out_xyz, float* out_desc, int* out_sid, long long* out_ids, void* stream) {
    PRAM_REQUIRE(row_frame && row_point && frame_cams && pt_ids && pt_xyz && pt_desc && pt_sid && pt_err && out_kpts && out_xyz && out_desc && out_sid &&
                 out_ids, "pram_compress_rows: null pointer");
    PRAM_REQUIRE(aligned(pt_desc, 16) && aligned(out_desc, 16), "pram_compress_rows: pt_desc and out_desc must be 16-byte aligned");
    PRAM_REQUIRE(aligned(frame_cams, 8) && aligned(pt_ids, 8) && aligned(pt_xyz, 8) && aligned(pt_err, 8) && aligned(out_kpts, 8) && aligned(out_xyz, 8) &&
                 aligned(out_ids, 8), "pram_compress_rows: 64-bit buffers must be 8-byte aligned");
    PRAM_REQUIRE(aligned(row_frame, 4) && aligned(row_point, 4) && aligned(pt_sid, 4) && aligned(out_sid, 4), "pram_compress_rows: misaligned pointer");
    PRAM_REQUIRE(n_out >= 0 && n_frames >= 1 && n_points >= 1, "pram_compress_rows: needs n_out >= 0, n_frames >= 1, n_points >= 1");
    if (n_out == 0) return PRAM_OK;
    hipLaunchKernelGGL(compress_rows_kernel, dim3((n_out + 7) / 8), dim3(256), 0, (hipStream_t)stream, row_frame, row_point, n_out, n_frames, n_points,
                       frame_cams, pt_ids, pt_xyz, reinterpret_cast<const float4*>(pt_desc), pt_sid, pt_err, out_kpts, out_xyz,
                       reinterpret_cast<float4*>(out_desc), out_sid, out_ids);
    return pram_launch_status("pram_compress_rows");
}
