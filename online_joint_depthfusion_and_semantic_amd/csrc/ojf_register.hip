// REGISTER: the rigid transform between two fused scenes of one room, by Gauss-Newton on signed distance fields - the
// voxels of the MOVING volume near its surface are points that carry their own distance, and the pose is sought under which
// the FIXED scene's field, read at the mapped points, shows the same distances.  Own definition (the reference has no
// counterpart); tests/register_ref.py restates it in numpy, and the GPU tests pin the selected list, J, r and the reason
// codes to it bit for bit and the fp64 sums / solve to 1e-12.
//
// Normative definition.  fp32 arithmetic has every product, sum and division rounded on its own (the build's
// -ffp-contract=off and correctly rounded division); "a + b + c" means (a + b) + c; lerp(a, b, f) = a + f·(b - a).
// Volumes are [X,Y,Z], linear index n = (i·Y + j)·Z + k; voxel (i,j,k) has its centre at origin + (i+0.5, j+0.5, k+0.5)·res.
// Origins and resolutions arrive as f64 on the host and are rounded once to fp32 (o_m, res_m of the moving volume, o_f, res_f
// of the fixed one); the estimated P = [R|t] maps points of the moving scene's world to the fixed scene's world.
// 1. Select.  Voxel (i,j,k) of the moving volume is a point iff i, j and k are multiples of `stride`, voxel_observed(T, W)
//   (ojf_blocks.h) and fabsf(fp32(T)) < band.  The points are the u32 linear indices in increasing order: blocks of 1024
//   consecutive voxels count theirs (lane t looks at voxels 4t..4t+3 of the block), block_exclusive_scan turns the counts into
//   offsets and writes the total, and a second sweep fills the list (entries past `capacity` are dropped).  No list: count only.
// 2. Associate, point n = (i,j,k) of the list (reason 1 for an n that is no voxel of the moving volume):
//   a_T = fp32(T_moving[n]); x_a = ((float)i_a + 0.5f)·res_m + o_m,a.
//   Pose P f64[12] in device memory, rounded once to fp32 (R, t): q_i = R[i0]·x0 + R[i1]·x1 + R[i2]·x2 + t_i.
//   g_a = (q_a - o_f,a)/res_f - 0.5f; fl_a = floorf(g_a).  reason 1 unless every g_a is finite and the cell is wholly inside
//   the fixed grid: 0 <= fl_a (and fl_a < 2^31, so that the integer i0_a = fl_a exists) and i0_a + 1 <= N_a - 1.
//   f_a = g_a - fl_a.  Corner v_{bx,by,bz} is voxel (i0_x+bx, i0_y+by, i0_z+bz) of the fixed field; it counts iff the voxel is
//   observed (TSDF form: v = fp32(T)) or its value is finite (f32 form).  reason 2 when a corner does not count; no value
//   of a non-counting corner is used.
//   dz_{bx,by} = v_{bx,by,1} - v_{bx,by,0};  e_{bx,by} = lerp(v_{bx,by,0}, v_{bx,by,1}, f_z);  e_{bx} = lerp(e_{bx,0}, e_{bx,1}, f_y);
//   F = lerp(e_0, e_1, f_x);  Gx = e_1 - e_0;  Gy = lerp(e_{0,1} - e_{0,0}, e_{1,1} - e_{1,0}, f_x);
//   Gz = lerp(lerp(dz_{0,0}, dz_{0,1}, f_y), lerp(dz_{1,0}, dz_{1,1}, f_y), f_x);  grad_a = G_a / res_f.
//   reason 3 unless fabsf(F) < field_band (the fixed field is saturated there; +inf for the f32 form).  r = F - a_T;
//   reason 4 unless fabsf(r) <= dist.  gg = (grad_x·grad_x + grad_y·grad_y) + grad_z·grad_z; reason 5 unless gg > 0 and
//   finite.  Otherwise reason 0, an inlier, with J = (q × grad, grad), the cross product in cross3's order (the left update
//   q' = q + w × q + tau of ojf_track).
//   Terms, block sums, rows, solve, stats, status codes and the freeze after a failed step are those of ojf_track (its header,
//   (b) last paragraph and (c); the code is shared through ojf_gauss_newton.h): 1024 points per block, lane t of a block takes
//   the points t, t + 256, t + 512, t + 768 of the block's 1024 in that order, one row per block; min_count =
//   min_inlier_fraction·n_points (fp64, host).
// Launches of ojf_register: one initialisation (P = E_init, status {0, -1}) unless the call continues from pose_dev, then per
// iteration one associate and one solve.  Kernel boundaries order the iterations; the host never waits.  No atomics, no inline
// assembly; every output is written once: the same bits on every run.  A wave's 64 points are consecutive entries of the list,
// which for a surface band is mostly runs along z of the moving volume: their corner loads fall into few cache lines.
#include "ojf_blocks.h"
#include "ojf_gauss_newton.h"

namespace ojf {

constexpr int kSelectThreads = 256;
constexpr int kSelectPerThread = 4;
constexpr int kSelectPerBlock = kSelectThreads * kSelectPerThread;

struct SelectArgs {
    const uint16_t *tsdf, *weights;
    int X, Y, Z, stride;
    float band;
    size_t nvox;
    uint32_t *counts;   // [blocks]: counts, then (after the scan) offsets
    uint32_t *list;     // or NULL
    uint32_t capacity;
};

__device__ __forceinline__ bool select_voxel(const SelectArgs &A, size_t n)
{
    const uint32_t v = (uint32_t)n, ij = v / (uint32_t)A.Z;  // (n < 2^31: 32-bit divisions)
    const uint32_t k = v - ij * (uint32_t)A.Z, i = ij / (uint32_t)A.Y, j = ij - i * (uint32_t)A.Y;
    if (i % (uint32_t)A.stride || j % (uint32_t)A.stride || k % (uint32_t)A.stride) return false;
    const uint16_t t = A.tsdf[n];
    return voxel_observed(t, A.weights[n]) && fabsf(h2f(t)) < A.band;
}

// FILL false: counts[block] = the block's points.  FILL true: the block's points go to list[counts[block] + ...] in index order.
template <bool FILL>
__global__ __launch_bounds__(kSelectThreads) void register_select_kernel(SelectArgs A)
{
    __shared__ uint32_t part[kSelectThreads];
    const size_t first = (size_t)blockIdx.x * kSelectPerBlock + (size_t)threadIdx.x * kSelectPerThread;
    uint32_t bits = 0, mine = 0;
#pragma unroll
    for (int e = 0; e < kSelectPerThread; ++e) {
        if (first + e < A.nvox && select_voxel(A, first + e)) {
            bits |= 1u << e;
            ++mine;
        }
    }
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < kSelectThreads; d <<= 1) {
        const uint32_t add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    if constexpr (!FILL) {
        if (threadIdx.x == kSelectThreads - 1) A.counts[blockIdx.x] = part[threadIdx.x];
    } else {
        uint64_t at = (uint64_t)A.counts[blockIdx.x] + (part[threadIdx.x] - mine);
#pragma unroll
        for (int e = 0; e < kSelectPerThread; ++e) {
            if (bits >> e & 1u) {
                if (at < A.capacity) A.list[at] = (uint32_t)(first + e);
                ++at;
            }
        }
    }
}

__global__ __launch_bounds__(kScanBlock) void register_scan_kernel(uint32_t *counts, uint32_t nblocks, uint32_t *count_out)
{
    const unsigned long long total = block_exclusive_scan<unsigned long long>(counts, counts, nblocks);
    if (threadIdx.x == 0) *count_out = (uint32_t)total;  // (at most X·Y·Z < 2^31)
}

struct RegisterArgs {
    const uint32_t *list;
    uint32_t n;
    const uint16_t *mtsdf;
    size_t mvox;
    int mY, mZ;
    float mres, mo[3];
    const uint16_t *ftsdf, *fweights;  // TSDF form
    const float *field;                // f32 form
    int fX, fY, fZ;
    float fres, fo[3];
    float field_band, dist;
    const double *pose;
    const int *status;
    double *rows;     // [blocks, 29]
    float *jr;        // [n, 7] or NULL
    uint8_t *reason;  // [n] or NULL
};

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

// corner value; false when the corner does not count
template <bool TSDF>
__device__ __forceinline__ bool field_corner(const RegisterArgs &A, size_t v, float &out)
{
    if constexpr (TSDF) {
        const uint16_t t = A.ftsdf[v];
        if (!voxel_observed(t, A.fweights[v])) return false;
        out = h2f(t);
        return true;
    } else {
        out = A.field[v];
        return fabsf(out) < INFINITY;
    }
}

// reason code of list entry `p`; for an inlier also J[6] and the residual
template <bool TSDF>
__device__ int associate_point(const RegisterArgs &A, const float R[9], const float t[3], uint32_t p, float J[6], float &res)
{
    const uint32_t n = A.list[p];
    if (n >= A.mvox) return 1;
    const uint32_t ij = n / (uint32_t)A.mZ, i = ij / (uint32_t)A.mY;
    const int idx[3] = {(int)i, (int)(ij - i * (uint32_t)A.mY), (int)(n - ij * (uint32_t)A.mZ)};
    const float aT = h2f(A.mtsdf[n]);
    float x[3], q[3], g[3], fl[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = ((float)idx[a] + 0.5f) * A.mres + A.mo[a];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2] + t[i];
    const int N[3] = {A.fX, A.fY, A.fZ};
    int i0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g[a] = (q[a] - A.fo[a]) / A.fres - 0.5f;
        fl[a] = floorf(g[a]);
    }
    if (!finite3(g)) return 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(fl[a] >= 0.0f && fl[a] < 2147483648.0f)) return 1;
        i0[a] = (int)fl[a];
        if ((int64_t)i0[a] + 1 > (int64_t)N[a] - 1) return 1;
    }
    const float fx = g[0] - fl[0], fy = g[1] - fl[1], fz = g[2] - fl[2];
    float v[2][2][2];
    bool all = true;
#pragma unroll
    for (int bx = 0; bx < 2; ++bx)
#pragma unroll
        for (int by = 0; by < 2; ++by)
#pragma unroll
            for (int bz = 0; bz < 2; ++bz) {
                const size_t c = ((size_t)(i0[0] + bx) * (size_t)A.fY + (size_t)(i0[1] + by)) * (size_t)A.fZ + (size_t)(i0[2] + bz);
                float val = 0.0f;
                all = field_corner<TSDF>(A, c, val) && all;
                v[bx][by][bz] = val;
            }
    if (!all) return 2;
    float dz[2][2], e2[2][2], e1[2];
#pragma unroll
    for (int bx = 0; bx < 2; ++bx) {
#pragma unroll
        for (int by = 0; by < 2; ++by) {
            dz[bx][by] = v[bx][by][1] - v[bx][by][0];
            e2[bx][by] = lerp(v[bx][by][0], v[bx][by][1], fz);
        }
        e1[bx] = lerp(e2[bx][0], e2[bx][1], fy);
    }
    const float F = lerp(e1[0], e1[1], fx);
    const float G[3] = {e1[1] - e1[0], lerp(e2[0][1] - e2[0][0], e2[1][1] - e2[1][0], fx),
                        lerp(lerp(dz[0][0], dz[0][1], fy), lerp(dz[1][0], dz[1][1], fy), fx)};
    const float grad[3] = {G[0] / A.fres, G[1] / A.fres, G[2] / A.fres};
    if (!(fabsf(F) < A.field_band)) return 3;
    const float r = F - aT;
    if (!(fabsf(r) <= A.dist)) return 4;
    const float gg = dot3(grad, grad);
    if (!(gg > 0.0f) || !(gg < INFINITY)) return 5;
    cross3(q, grad, J);
    J[3] = grad[0];
    J[4] = grad[1];
    J[5] = grad[2];
    res = r;
    return 0;
}

template <bool TSDF>
__global__ __launch_bounds__(kTrackThreads) void register_associate_kernel(RegisterArgs A)
{
    if (A.status[0] != 0) return;  // a failed step froze the pose: nothing more to do (uniform over the grid)
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) R[3 * i + k] = (float)A.pose[4 * i + k];
        t[i] = (float)A.pose[4 * i + 3];
    }
    double acc[kTrackTerms];
#pragma unroll
    for (int e = 0; e < kTrackTerms; ++e) acc[e] = 0.0;
    for (int k = 0; k < kTrackPixPerThread; ++k) {
        const uint64_t p = (uint64_t)blockIdx.x * kTrackPixPerBlock + (uint64_t)(k * kTrackThreads) + threadIdx.x;
        if (p >= A.n) break;
        float J[6] = {0, 0, 0, 0, 0, 0}, res = 0.0f;
        const int why = associate_point<TSDF>(A, R, t, (uint32_t)p, J, res);
        if (A.reason) A.reason[p] = (uint8_t)why;
        if (A.jr) {
#pragma unroll
            for (int i = 0; i < 6; ++i) A.jr[7 * (size_t)p + i] = why ? 0.0f : J[i];
            A.jr[7 * (size_t)p + 6] = why ? 0.0f : res;
        }
        if (why) continue;
        add_terms(acc, J, res);
    }
    block_terms_to_row(acc, A.rows + (size_t)blockIdx.x * kTrackTerms);
}

struct RegisterInit {
    double *pose;
    int *status;
    double init[12];
};

__global__ void register_init_kernel(RegisterInit I)
{
    if (threadIdx.x < 12) I.pose[threadIdx.x] = I.init[threadIdx.x];
    if (threadIdx.x == 0) {
        I.status[0] = 0;
        I.status[1] = -1;
    }
}

static uint32_t point_blocks(size_t n) { return (uint32_t)((n + kTrackPixPerBlock - 1) / kTrackPixPerBlock); }

// rows of the associate blocks (which covers the select counts: 4 bytes per 1024 voxels) | 256 bytes of scratch
static size_t register_workspace(size_t n) { return align256((size_t)point_blocks(n) * kTrackTerms * sizeof(double)) + 256; }

static bool misaligned(const void *p, size_t a) { return ((uintptr_t)p % a) != 0; }

static int check_box(const char *who, const char *which, int X, int Y, int Z, const double *origin, double res)
{
    const std::string w = std::string(who) + ": " + which;
    if (X <= 0 || Y <= 0 || Z <= 0) return fail(w + ": non-positive volume size");
    if (!volume_size_ok(X, Y, Z)) return fail(w + ": volume too large");
    if (!origin) return fail(w + ": null pointer argument (origin)");
    if (!all_finite(origin, 3)) return fail(w + ": non-finite origin");
    if (!(res > 0.0) || !std::isfinite(res) || !((float)res > 0.0f) || !std::isfinite((float)res))
        return fail(w + ": resolution must be > 0 and finite");
    return 0;
}

struct RegisterScene {  // what ojf_register and ojf_register_associate share of their arguments
    const uint16_t *mtsdf;
    int mX, mY, mZ;
    const double *mo;
    double mres;
    const uint32_t *list;
    uint32_t n;
    const uint16_t *ftsdf, *fweights;
    const float *field;
    int fX, fY, fZ;
    const double *fo;
    double fres, field_band, dist, frac;
};

static int check_scene(const char *who, const RegisterScene &S)
{
    if (int rc = check_box(who, "moving", S.mX, S.mY, S.mZ, S.mo, S.mres)) return rc;
    if (int rc = check_box(who, "fixed", S.fX, S.fY, S.fZ, S.fo, S.fres)) return rc;
    if (!S.mtsdf) return refuse(who, "null pointer argument (moving_tsdf_dev)");
    if (!S.list) return refuse(who, "null pointer argument (list_dev)");
    if (S.n == 0) return refuse(who, "n_points must be at least 1");
    if ((size_t)S.n > (size_t)S.mX * S.mY * S.mZ) return refuse(who, "n_points exceeds the moving volume");
    if (S.field) {
        if (S.ftsdf || S.fweights) return refuse(who, "fixed_field_dev excludes fixed_tsdf_dev / fixed_weights_dev");
    } else if (!S.ftsdf || !S.fweights) {
        return refuse(who, "null pointer argument (fixed_tsdf_dev and fixed_weights_dev, or fixed_field_dev)");
    }
    if (!(S.field_band > 0.0)) return refuse(who, "field_band must be > 0");
    if (!(S.dist > 0.0) || !std::isfinite(S.dist)) return refuse(who, "dist must be > 0 and finite");
    if (!(S.frac >= 0.0) || !(S.frac <= 1.0)) return refuse(who, "min_inlier_fraction must be in 0..1");
    if (misaligned(S.mtsdf, 2) || misaligned(S.ftsdf, 2) || misaligned(S.fweights, 2))
        return refuse(who, "misaligned pointer (fp16 volumes: 2 bytes)");
    if (misaligned(S.list, 4) || misaligned(S.field, 4)) return refuse(who, "misaligned pointer (list_dev, fixed_field_dev: 4 bytes)");
    return 0;
}

static int check_outputs(const char *who, const void *ws, size_t ws_bytes, size_t n, const double *pose, const void *f64_out,
                         const int *status)
{
    if (!ws || !pose || !f64_out || !status) return refuse(who, "null pointer argument (workspace, pose, stats / sums, status)");
    if (misaligned(ws, 8) || misaligned(pose, 8) || misaligned(f64_out, 8) || misaligned(status, 4))
        return refuse(who, "misaligned pointer (workspace_dev, pose_dev, stats_dev / sums_dev: 8 bytes, status_dev: 4)");
    if (ws_bytes < register_workspace(n)) return refuse(who, "workspace too small");
    return 0;
}

static void fill_register(RegisterArgs &A, const RegisterScene &S, const double *pose, const int *status, double *rows)
{
    A.list = S.list; A.n = S.n; A.mtsdf = S.mtsdf; A.mvox = (size_t)S.mX * S.mY * S.mZ; A.mY = S.mY; A.mZ = S.mZ;
    A.mres = (float)S.mres;
    A.ftsdf = S.ftsdf; A.fweights = S.fweights; A.field = S.field;
    A.fX = S.fX; A.fY = S.fY; A.fZ = S.fZ;
    A.fres = (float)S.fres;
    for (int a = 0; a < 3; ++a) {
        A.mo[a] = (float)S.mo[a];
        A.fo[a] = (float)S.fo[a];
    }
    A.field_band = (float)S.field_band;
    A.dist = (float)S.dist;
    A.pose = pose; A.status = status; A.rows = rows;
    A.jr = nullptr; A.reason = nullptr;
}

static int launch_init(double *pose, int *status, const double *init, hipStream_t s)
{
    RegisterInit I;
    I.pose = pose; I.status = status;
    for (int i = 0; i < 12; ++i) I.init[i] = init[i];
    hipLaunchKernelGGL(register_init_kernel, dim3(1), dim3(64), 0, s, I);
    OJF_HIP(hipGetLastError());
    return 0;
}

static int launch_register_step(const RegisterArgs &A, const SolveArgs &S, hipStream_t s)
{
    if (A.field) hipLaunchKernelGGL(register_associate_kernel<false>, dim3(S.nblocks), dim3(kTrackThreads), 0, s, A);
    else hipLaunchKernelGGL(register_associate_kernel<true>, dim3(S.nblocks), dim3(kTrackThreads), 0, s, A);
    OJF_HIP(hipGetLastError());
    return launch_solve(S, s);
}

}  // namespace ojf

OJF_API size_t ojf_register_workspace_bytes(size_t n)
{
    using namespace ojf;
    if (n == 0 || n > 0x7fffffffULL) return 0;
    return register_workspace(n);
}

OJF_API int ojf_register_select(const uint16_t *tsdf_dev, const uint16_t *weights_dev, int X, int Y, int Z, float band, int stride,
                                void *workspace_dev, size_t workspace_bytes, uint32_t *list_dev, uint32_t capacity,
                                uint32_t *count_dev, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_register_select";
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    if (!tsdf_dev || !weights_dev || !workspace_dev || !count_dev) return refuse(who, "null pointer argument");
    if (stride < 1) return refuse(who, "stride must be at least 1");
    if (!(band > 0.0f)) return refuse(who, "band must be > 0");
    if (misaligned(tsdf_dev, 2) || misaligned(weights_dev, 2) || misaligned(workspace_dev, 4) || misaligned(list_dev, 4) ||
        misaligned(count_dev, 4))
        return refuse(who, "misaligned pointer (fp16 volumes: 2 bytes; workspace_dev, list_dev, count_dev: 4)");
    const size_t nvox = (size_t)X * Y * Z;
    if (workspace_bytes < register_workspace(nvox)) return refuse(who, "workspace too small");
    SelectArgs A;
    A.tsdf = tsdf_dev; A.weights = weights_dev; A.X = X; A.Y = Y; A.Z = Z; A.stride = stride; A.band = band; A.nvox = nvox;
    A.counts = (uint32_t *)workspace_dev; A.list = list_dev; A.capacity = capacity;
    const uint32_t blocks = (uint32_t)((nvox + kSelectPerBlock - 1) / kSelectPerBlock);
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(register_select_kernel<false>, dim3(blocks), dim3(kSelectThreads), 0, s, A);
    OJF_HIP(hipGetLastError());
    hipLaunchKernelGGL(register_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, A.counts, blocks, count_dev);
    OJF_HIP(hipGetLastError());
    if (list_dev && capacity) {
        hipLaunchKernelGGL(register_select_kernel<true>, dim3(blocks), dim3(kSelectThreads), 0, s, A);
        OJF_HIP(hipGetLastError());
    }
    return 0;
}

OJF_API int ojf_register(const uint16_t *moving_tsdf_dev, int mX, int mY, int mZ, const double *moving_origin_host,
                         double moving_resolution, const uint32_t *list_dev, uint32_t n_points, const uint16_t *fixed_tsdf_dev,
                         const uint16_t *fixed_weights_dev, const float *fixed_field_dev, int fX, int fY, int fZ,
                         const double *fixed_origin_host, double fixed_resolution, double field_band, double dist,
                         int iterations, int first_iteration, double min_inlier_fraction, const double *E_init_host,
                         int continue_from_pose, void *workspace_dev, size_t workspace_bytes, double *pose_dev, double *stats_dev,
                         int *status_dev, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_register";
    const RegisterScene sc = {moving_tsdf_dev, mX, mY, mZ, moving_origin_host, moving_resolution, list_dev, n_points,
                              fixed_tsdf_dev, fixed_weights_dev, fixed_field_dev, fX, fY, fZ, fixed_origin_host, fixed_resolution,
                              field_band, dist, min_inlier_fraction};
    if (int rc = check_scene(who, sc)) return rc;
    if (!E_init_host) return refuse(who, "null pointer argument (E_init_host)");
    if (!all_finite(E_init_host, 12)) return refuse(who, "non-finite E_init_host");
    if (iterations < 0 || first_iteration < 0 || (int64_t)iterations + first_iteration > OJF_REGISTER_MAX_ITERATIONS)
        return refuse(who, "iterations: first_iteration + iterations must be within 0..OJF_REGISTER_MAX_ITERATIONS");
    if (int rc = check_outputs(who, workspace_dev, workspace_bytes, n_points, pose_dev, stats_dev, status_dev)) return rc;
    const hipStream_t s = as_stream(stream);
    if (!continue_from_pose)
        if (int rc = launch_init(pose_dev, status_dev, E_init_host, s)) return rc;
    RegisterArgs A;
    fill_register(A, sc, pose_dev, status_dev, (double *)workspace_dev);
    SolveArgs S;
    fill_solve(S, A.rows, (int)point_blocks(n_points), pose_dev, status_dev, stats_dev, nullptr, 0,
               min_inlier_fraction * (double)n_points, E_init_host);
    for (int k = 0; k < iterations; ++k) {
        S.iter = first_iteration + k;
        if (int rc = launch_register_step(A, S, s)) return rc;
    }
    return 0;
}

OJF_API int ojf_register_associate(const uint16_t *moving_tsdf_dev, int mX, int mY, int mZ, const double *moving_origin_host,
                                   double moving_resolution, const uint32_t *list_dev, uint32_t n_points,
                                   const uint16_t *fixed_tsdf_dev, const uint16_t *fixed_weights_dev, const float *fixed_field_dev,
                                   int fX, int fY, int fZ, const double *fixed_origin_host, double fixed_resolution,
                                   double field_band, double dist, double min_inlier_fraction, const double *E_pose_host,
                                   void *workspace_dev, size_t workspace_bytes, double *pose_dev, double *sums_dev, float *jr_dev,
                                   uint8_t *reason_dev, int *status_dev, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_register_associate";
    const RegisterScene sc = {moving_tsdf_dev, mX, mY, mZ, moving_origin_host, moving_resolution, list_dev, n_points,
                              fixed_tsdf_dev, fixed_weights_dev, fixed_field_dev, fX, fY, fZ, fixed_origin_host, fixed_resolution,
                              field_band, dist, min_inlier_fraction};
    if (int rc = check_scene(who, sc)) return rc;
    if (!E_pose_host) return refuse(who, "null pointer argument (E_pose_host)");
    if (!all_finite(E_pose_host, 12)) return refuse(who, "non-finite E_pose_host");
    if (int rc = check_outputs(who, workspace_dev, workspace_bytes, n_points, pose_dev, sums_dev, status_dev)) return rc;
    if (misaligned(jr_dev, 4)) return refuse(who, "misaligned pointer (jr_dev: 4 bytes)");
    const hipStream_t s = as_stream(stream);
    if (int rc = launch_init(pose_dev, status_dev, E_pose_host, s)) return rc;
    RegisterArgs A;
    fill_register(A, sc, pose_dev, status_dev, (double *)workspace_dev);
    A.jr = jr_dev;
    A.reason = reason_dev;
    double *stats = (double *)((char *)workspace_dev + register_workspace(n_points) - 256);  // the stats row goes to the scratch tail
    SolveArgs S;
    fill_solve(S, A.rows, (int)point_blocks(n_points), pose_dev, status_dev, stats, sums_dev, 0,
               min_inlier_fraction * (double)n_points, E_pose_host);
    return launch_register_step(A, S, s);
}
