// The front half that ojf_track.hip (depth only) and ojf_track_rgbd.hip (depth and colour) share, defined once: the depth
// pyramid, the level camera, the geometric association as stages, the row export, the host checks and the level-by-iteration
// launch loop.  The normative text is (a) and (b) of ojf_track.hip's header.  The two associate kernels keep their own control
// flow (ojf_track.hip leaves a pixel at its first failed test; ojf_track_rgbd.hip projects every pixel with depth and issues
// the model loads together) and call the same stages: with -ffp-contract=off every product, sum, division and sqrt rounds on
// its own, so the same expressions give the same bits in either order of tests.  Nothing here may be reassociated.
// Everything is `static` or a template: two translation units include it.
#pragma once
#include "ojf_gauss_newton.h"

#include <type_traits>

namespace ojf {

// ---- (a) the depth pyramid
struct DepthSource {
    const float *depth;
    const uint8_t *mask;
    int w;
    float delta;
};

__device__ __forceinline__ float depth_level0(const DepthSource &S, int r, int c)
{
    const size_t i = (size_t)r * S.w + c;
    const float d = S.depth[i];
    const bool ok = isfinite(d) && d > 0.0f && (!S.mask || S.mask[i] != 0);
    return ok ? d : 0.0f;
}

__device__ __forceinline__ float depth_block(const float v[4], float delta)
{
    float dmin = INFINITY;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v[k] != 0.0f) {
            dmin = fminf(dmin, v[k]);
            any = true;
        }
    }
    if (!any) return 0.0f;
    float s = 0.0f;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v[k] != 0.0f && (v[k] - dmin) <= delta) {
            s = s + v[k];
            ++n;
        }
    }
    return s / (float)n;
}

template <int LV>
__device__ float depth_pyramid_value(const DepthSource &S, int r, int c)
{
    if constexpr (LV == 0) {
        return depth_level0(S, r, c);
    } else {
        const float v[4] = {depth_pyramid_value<LV - 1>(S, 2 * r, 2 * c), depth_pyramid_value<LV - 1>(S, 2 * r, 2 * c + 1),
                            depth_pyramid_value<LV - 1>(S, 2 * r + 1, 2 * c), depth_pyramid_value<LV - 1>(S, 2 * r + 1, 2 * c + 1)};
        return depth_block(v, S.delta);
    }
}

// f(std::integral_constant<int, l>) for the run-time level l: the one switch over OJF_TRACK_MAX_LEVELS
template <class F>
__device__ __forceinline__ void with_level(int l, F &&f)
{
    static_assert(OJF_TRACK_MAX_LEVELS == 4, "one case per level");
    switch (l) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
    }
}

// what a pyramid / prepare launch leaves besides its images: P = E_init, status {0, -1}
__device__ __forceinline__ void write_initial_state(double *pose, int *status, const double init[12])
{
    for (int i = 0; i < 12; ++i) pose[i] = init[i];
    status[0] = 0;
    status[1] = -1;
}

// ---- (b) the camera of one level and the stages of the geometric association
struct LevelCamera {
    int h, w, npix;
    float Ki[9];
    float fx, fy, cx, cy;
    float Rr[9], tr[3];
    float dist2, cos_thr;
};

__device__ __forceinline__ void ray_dc(const float Ki[9], int r, int c, float dc[3])
{
    const float cf = (float)c, rf = (float)r;
#pragma unroll
    for (int i = 0; i < 3; ++i) dc[i] = Ki[3 * i] * cf + Ki[3 * i + 1] * rf + Ki[3 * i + 2];
}

__device__ __forceinline__ void vertex(const LevelCamera &C, int r, int c, float D, float V[3])
{
    float dc[3];
    ray_dc(C.Ki, r, c, dc);
#pragma unroll
    for (int i = 0; i < 3; ++i) V[i] = D * dc[i];
}

// n_c of pixel (r, c) with vertex v from the depths below and to the right of it (both non-zero); false, n untouched, when
// the cross product has no length
__device__ __forceinline__ bool live_normal(const LevelCamera &C, int r, int c, const float v[3], float Dd, float Dr, float n[3])
{
    float vd[3], vr[3], a[3], b[3];
    vertex(C, r + 1, c, Dd, vd);
    vertex(C, r, c + 1, Dr, vr);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i] = vd[i] - v[i];
        b[i] = vr[i] - v[i];
    }
    const float x[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const float xx = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (!(xx > 0.0f) || !isfinite(xx)) return false;
    const float xl = sqrtf(xx);
    n[0] = x[0] / xl;
    n[1] = x[1] / xl;
    n[2] = x[2] / xl;
    return true;
}

// p and nw in the world by the pose (R, t); q = p in the reference camera
__device__ __forceinline__ void pose_transform(const LevelCamera &C, const float R[9], const float t[3], const float v[3],
                                               const float n[3], float p[3], float nw[3], float q[3])
{
    float e[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2] + t[i];
        nw[i] = R[3 * i] * n[0] + R[3 * i + 1] * n[1] + R[3 * i + 2] * n[2];
        e[i] = p[i] - C.tr[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = C.Rr[i] * e[0] + C.Rr[3 + i] * e[1] + C.Rr[6 + i] * e[2];
}

// 0 with (ux, uy) and the nearest model pixel (fr, fc), 3 behind the reference camera (nothing written), 4 outside its image
__device__ __forceinline__ int project(const LevelCamera &C, const float q[3], float &ux, float &uy, float &fc, float &fr)
{
    if (!(q[2] > 0.0f)) return 3;
    ux = C.fx * (q[0] / q[2]) + C.cx;
    uy = C.fy * (q[1] / q[2]) + C.cy;
    fc = floorf(ux + 0.5f);
    fr = floorf(uy + 0.5f);
    return fc >= 0.0f && fc < (float)C.w && fr >= 0.0f && fr < (float)C.h ? 0 : 4;
}

// g = p - m for the model point m of depth dm at (mr, mc); false when it is farther than the distance threshold
__device__ __forceinline__ bool model_gap(const LevelCamera &C, const float p[3], int mr, int mc, float dm, float g[3])
{
    float mv[3];
    vertex(C, mr, mc, dm, mv);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float m = C.Rr[3 * i] * mv[0] + C.Rr[3 * i + 1] * mv[1] + C.Rr[3 * i + 2] * mv[2] + C.tr[i];
        g[i] = p[i] - m;
    }
    return !(g[0] * g[0] + g[1] * g[1] + g[2] * g[2] > C.dist2);
}

__device__ __forceinline__ bool normals_agree(const LevelCamera &C, const float nw[3], const float nm[3])
{
    return !(nw[0] * nm[0] + nw[1] * nm[1] + nw[2] * nm[2] < C.cos_thr);
}

// the point-to-plane row: J = (p x n_m, n_m), r = n_m . g
__device__ __forceinline__ void plane_row(const float p[3], const float nm[3], const float g[3], float J[6], float &res)
{
    res = nm[0] * g[0] + nm[1] * g[1] + nm[2] * g[2];
    J[0] = p[1] * nm[2] - p[2] * nm[1];
    J[1] = p[2] * nm[0] - p[0] * nm[2];
    J[2] = p[0] * nm[1] - p[1] * nm[0];
    J[3] = nm[0];
    J[4] = nm[1];
    J[5] = nm[2];
}

// ---- what the two associate kernels do around their pixels
__device__ __forceinline__ void load_pose_f32(const double *pose, float R[9], float t[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) R[3 * i + k] = (float)pose[4 * i + k];
        t[i] = (float)pose[4 * i + 3];
    }
}

// the probe's exports of one pixel (either may be NULL): its reason byte, and its row, 0 unless the reason is 0
__device__ __forceinline__ void export_row(uint8_t *reason, float *jr, int pix, int why, const float J[6], float res)
{
    if (reason) reason[pix] = (uint8_t)why;
    if (jr) {
#pragma unroll
        for (int i = 0; i < 6; ++i) jr[7 * (size_t)pix + i] = why ? 0.0f : J[i];
        jr[7 * (size_t)pix + 6] = why ? 0.0f : res;
    }
}

// ---- host: sizes, checks, the camera fill and the launch loop
static int level_blocks(int h, int w, int l) { return (((h >> l) * (w >> l)) + kTrackPixPerBlock - 1) / kTrackPixPerBlock; }

static size_t total_pixels(int h, int w, int levels)
{
    size_t n = 0;
    for (int l = 0; l < levels; ++l) n += (size_t)(h >> l) * (size_t)(w >> l);
    return n;
}

static size_t pyramid_bytes(int h, int w, int levels) { return align256(total_pixels(h, w, levels) * sizeof(float)); }

// the block rows of the largest level and the 256 bytes behind them (the probe's stats row): the tail of either workspace
static size_t rows_bytes(int h, int w) { return align256((size_t)level_blocks(h, w, 0) * kTrackTerms * sizeof(double)) + 256; }

// what a workspace size can be computed for (check_shape asks for more)
static bool sizable(int h, int w, int levels)
{
    return levels >= 1 && levels <= OJF_TRACK_MAX_LEVELS && h > 0 && w > 0 && (int64_t)h * w <= 0x3fffffffLL;
}

static int check_shape(const char *who, int h, int w, int levels)
{
    if (levels < 1 || levels > OJF_TRACK_MAX_LEVELS) return fail(std::string(who) + ": levels must be 1..OJF_TRACK_MAX_LEVELS");
    if (h <= 0 || w <= 0 || (int64_t)h * w > 0x3fffffffLL) return fail(std::string(who) + ": bad image size");
    if ((h >> (levels - 1)) < 8 || (w >> (levels - 1)) < 8)
        return fail(std::string(who) + ": every level must be at least 8 x 8 pixels");
    return 0;
}

// every level's model images are there and the iteration counts are legal; maps: one array of `levels` pointers per image
template <class... T>
static int check_schedule(const char *who, int levels, const int *iterations, const T *const *... maps)
{
    int total = 0;
    for (int l = 0; l < levels; ++l) {
        if ((... || !maps[l])) return fail(std::string(who) + ": null pointer argument (model maps)");
        if (iterations[l] < 0) return fail(std::string(who) + ": negative iteration count");
        total += iterations[l];
        if (total > OJF_TRACK_MAX_ITERATIONS) return fail(std::string(who) + ": more than OJF_TRACK_MAX_ITERATIONS iterations");
    }
    return 0;
}

// the thresholds both trackers take
static bool thresholds_in_range(double dist, double angle, double delta, double frac)
{
    return dist > 0.0 && isfinite(dist) && angle > 0.0 && angle <= 180.0 && delta >= 0.0 && isfinite(delta) && frac >= 0.0 &&
           frac <= 1.0;
}

// K: the level-0 intrinsics f64[9]; Ki: Kinv_l as the caller formed it
static void fill_camera(LevelCamera &C, int h, int w, int l, const double *K, const float *Ki, const double *Eref, double dist,
                        double angle)
{
    C.h = h >> l; C.w = w >> l; C.npix = C.h * C.w;
    for (int i = 0; i < 9; ++i) C.Ki[i] = Ki[i];
    const double s = (double)(1 << l);
    C.fx = (float)(K[0] / s);
    C.fy = (float)(K[4] / s);
    C.cx = (float)((K[2] + 0.5) / s - 0.5);
    C.cy = (float)((K[5] + 0.5) / s - 0.5);
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) C.Rr[3 * i + k] = (float)Eref[4 * i + k];
        C.tr[i] = (float)Eref[4 * i + 3];
    }
    C.dist2 = (float)(dist * dist);
    C.cos_thr = (float)cos(angle * M_PI / 180.0);
}

// Per level from levels-1 down to 0 and per iteration: associate(l, blocks) launches that level's associate kernel, then the
// solve.  stats row k belongs to the k-th step; sums (or NULL) receives the 29 sums of every step.
template <class Associate>
static int run_steps(int h, int w, int levels, const int *iterations, double min_inlier_fraction, double *rows, double *pose,
                     int *status, double *stats, double *sums, const double *init, hipStream_t s, Associate &&associate)
{
    int iter = 0;
    for (int l = levels - 1; l >= 0; --l) {
        SolveArgs S;
        fill_solve(S, rows, level_blocks(h, w, l), pose, status, stats, sums, 0,
                   min_inlier_fraction * (double)((h >> l) * (w >> l)), init);
        for (int k = 0; k < iterations[l]; ++k) {
            S.iter = iter++;
            if (int rc = associate(l, S.nblocks)) return rc;
            if (int rc = launch_solve(S, s)) return rc;
        }
    }
    return 0;
}

}  // namespace ojf
