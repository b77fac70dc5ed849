// TRACK RGBD: frame-to-model tracking with a photometric term beside the point-to-plane term of ojf_track.hip (the joint
// residual of Kintinuous / ElasticFusion): the live colour image is compared with colour images of the model
// (ojf_color_render at the depths of the model's ray casts), which pins the degrees of freedom geometry leaves open on a
// plane.  Own definition; tests/track_rgbd_ref.py restates it in numpy, and the GPU tests pin both pyramids, the model maps,
// J, r and the reason codes of both terms to it bit for bit and the fp64 sums / solve to 1e-12.
//
// Normative definition.  Rounding, "a + b + c", the levels, the level intrinsics fx_l .. cy_l, Ki, dc(r, c), the depth
// pyramid (a), the association (b) with its reason codes 1..7, J and r, the 29 terms, the block sums and the solve (c) are
// ojf_track.hip's, and so is their code: (a), the stages of (b), the row export, the host checks and the launch loop are in
// ojf_track_front.h, the terms and (c) in ojf_gauss_newton.h; the associate kernel here calls the stages in its own order
// (every pixel with depth is projected; the model loads are issued together).  The same inputs give the same bits.  What is
// added, and all that namespace rgbd holds:
// (d) Intensity of an RGBA byte quadruple: I = (float)(77·R + 150·G + 29·B) / 256.0f (the integer is at most 65280: the
//   conversion and the division are exact).  Live pyramid: I_0 from the live image (its fourth byte is ignored);
//   I_{l+1}(r, c) = (((a + b) + c) + d)·0.25f over (I_l(2r,2c), I_l(2r,2c+1), I_l(2r+1,2c), I_l(2r+1,2c+1)).  It does not
//   depend on the depth or the mask.
// (e) Model map of level l, one record (I_m, gx, gy, valid) of four floats per pixel, from the level's model colour image
//   (u8 RGBA, alpha 0: no intensity) and model depth d.  I_m = the intensity where alpha != 0, else 0.  The gradient is valid
//   (valid = 1.0f) when 1 <= r <= h_l - 2 and 1 <= c <= w_l - 2, the pixel and its four axis neighbours have alpha != 0, and
//   fabsf(d(neighbour) - d(r, c)) <= grad_depth for each of the four (a NaN fails); then gx = (I(r, c+1) - I(r, c-1))·0.5f,
//   gy = (I(r+1, c) - I(r-1, c))·0.5f.  Otherwise gx = gy = valid = 0.  (host: grad_depth = fp32(grad_depth_limit).)
// (f) Photometric row of live pixel (r, c) of level l at the current pose.  lambda = fp32(photo_weight); when lambda == 0
//   the photometric reason of every pixel is 10 and nothing below is evaluated.  Otherwise, with v, p, q, ux, uy, (row, col),
//   d_m, g of (b), which are evaluated whether or not the pixel has a normal, the photometric reason is the first of
//   1 (D == 0), 3 (not q2 > 0), 4 (outside the model image), 5 (d_m == 0), 6 (too far) that applies - the checks of (b) but
//   the two on normals, so a pixel with geometric reason 0, 2 or 7 passes them all.  Then x0 = floor(ux), y0 = floor(uy),
//   ax = ux - x0, ay = uy - y0; reason 8 unless 0 <= x0 <= w_l - 2, 0 <= y0 <= h_l - 2 and the records at (y0, x0),
//   (y0, x0+1), (y0+1, x0), (y0+1, x0+1) all have valid != 0.  Each of I_m, gx, gy is interpolated as
//   top = v00 + ax·(v01 - v00), bot = v10 + ax·(v11 - v10), value = top + ay·(bot - top).
//   r_I = I_m - I_l(r, c); reason 9 unless fabsf(r_I) <= fp32(photo_thresh) (a hard cut).  Otherwise reason 0:
//   a0 = fx_l·gx, a1 = fy_l·gy; g_c = (a0 / q2, a1 / q2, -((a0·q0 + a1·q1) / (q2·q2)));
//   a_i = Rr[i0]·g_c0 + Rr[i1]·g_c1 + Rr[i2]·g_c2;  J_I = (p × a, a) with the cross product of (b).
// (g) Terms.  A pixel adds the terms of its geometric row (J, r) when its geometric reason is 0, then those of
//   (lambda·J_I_i, lambda·r_I) (each product rounded to fp32) when its photometric reason is 0; term 28 counts the pixel
//   once.  Summation order and the one row of 29 per block of 1024 pixels are (b)'s.
// Launches: one prepare (both pyramids, the model maps of every level, P = E_init, status {0, -1}), then per level from L-1
// down to 0 and per iteration one associate and one shared solve: 1 + 2·sum(iterations).  The host never waits.  No atomics,
// no inline assembly; every output is written once: the same bits on every run.
#include "ojf_track_front.h"

namespace ojf {
namespace rgbd {

constexpr int kTileW = 32, kTileH = 8;  // the prepare tile (ojf_frames.hip's); 34 x 10 with its halo

struct PrepArgs {
    const float *depth;
    const uint8_t *mask;
    const uint32_t *image;                          // live RGBA [h, w]
    float *dpyr, *ipyr;                             // levels back to back
    float4 *maps;                                   // likewise
    const float *mdepth[OJF_TRACK_MAX_LEVELS];      // NULL with mcolor: no map at that level
    const uint32_t *mcolor[OJF_TRACK_MAX_LEVELS];
    int h, w, levels;
    int off[OJF_TRACK_MAX_LEVELS + 1];              // pixel offset of level l (off[levels] = total)
    int tile0[OJF_TRACK_MAX_LEVELS + 1];            // first block of level l (tile0[levels] = grid size)
    float delta, grad_depth;
    double *pose;
    int *status;
    double init[12];
};

__device__ __forceinline__ float intensity_of(uint32_t rgba)
{
    const int v = 77 * (int)(rgba & 255u) + 150 * (int)((rgba >> 8) & 255u) + 29 * (int)((rgba >> 16) & 255u);
    return (float)v / 256.0f;
}

template <int LV>
__device__ float intensity_value(const PrepArgs &A, int r, int c)
{
    if constexpr (LV == 0) {
        return intensity_of(A.image[(size_t)r * A.w + c]);
    } else {
        const float a = intensity_value<LV - 1>(A, 2 * r, 2 * c), b = intensity_value<LV - 1>(A, 2 * r, 2 * c + 1);
        const float d = intensity_value<LV - 1>(A, 2 * r + 1, 2 * c), e = intensity_value<LV - 1>(A, 2 * r + 1, 2 * c + 1);
        return (((a + b) + d) + e) * 0.25f;
    }
}

// One block per 32 x 8 tile of one level; thread (lr, lc) owns pixel (r0 + lr, c0 + lc) and writes its depth pyramid value,
// its intensity pyramid value and its model map record.  The tile's model intensity (-1: none) and model depth sit in LDS
// with a one-pixel halo; each 32-lane half of a wave reads 32 consecutive floats of one tile row: no bank conflicts.
__global__ __launch_bounds__(kTileW *kTileH) void track_rgbd_prepare_kernel(PrepArgs A)
{
    __shared__ float sI[kTileH + 2][kTileW + 2];
    __shared__ float sD[kTileH + 2][kTileW + 2];
    const int t = (int)threadIdx.x;
    if (blockIdx.x == 0 && t == 0) write_initial_state(A.pose, A.status, A.init);
    int l = 0;
    while (l + 1 < A.levels && (int)blockIdx.x >= A.tile0[l + 1]) ++l;
    const int hl = A.h >> l, wl = A.w >> l;
    const int tiles_x = (wl + kTileW - 1) / kTileW;
    const int tb = (int)blockIdx.x - A.tile0[l];
    const int r0 = (tb / tiles_x) * kTileH, c0 = (tb % tiles_x) * kTileW;
    const uint32_t *mcolor = A.mcolor[l];
    const float *mdepth = A.mdepth[l];
    if (mcolor) {  // (uniform over the block)
        for (int i = t; i < (kTileH + 2) * (kTileW + 2); i += kTileW * kTileH) {
            const int hr = i / (kTileW + 2), hc = i % (kTileW + 2);
            const int rr = r0 + hr - 1, cc = c0 + hc - 1;
            float I = -1.0f, d = 0.0f;
            if (rr >= 0 && rr < hl && cc >= 0 && cc < wl) {
                const size_t j = (size_t)rr * wl + cc;
                const uint32_t px = mcolor[j];
                d = mdepth[j];
                if (px >> 24) I = intensity_of(px);
            }
            sI[hr][hc] = I;
            sD[hr][hc] = d;
        }
    }
    __syncthreads();
    const int lr = t / kTileW, lc = t % kTileW;
    const int r = r0 + lr, c = c0 + lc;
    if (r >= hl || c >= wl) return;
    const size_t g = (size_t)A.off[l] + (size_t)r * wl + c;
    const DepthSource S = {A.depth, A.mask, A.w, A.delta};
    float d, I;
    with_level(l, [&](auto lv) {
        d = depth_pyramid_value<decltype(lv)::value>(S, r, c);
        I = intensity_value<decltype(lv)::value>(A, r, c);
    });
    A.dpyr[g] = d;
    A.ipyr[g] = I;
    if (!mcolor) return;
    const int y = lr + 1, x = lc + 1;
    const float Ic = sI[y][x], Il = sI[y][x - 1], Ir = sI[y][x + 1], Iu = sI[y - 1][x], Id = sI[y + 1][x];
    const float dc = sD[y][x];
    bool ok = r >= 1 && r <= hl - 2 && c >= 1 && c <= wl - 2;
    ok = ok && Ic >= 0.0f && Il >= 0.0f && Ir >= 0.0f && Iu >= 0.0f && Id >= 0.0f;
    ok = ok && fabsf(sD[y][x - 1] - dc) <= A.grad_depth && fabsf(sD[y][x + 1] - dc) <= A.grad_depth &&
         fabsf(sD[y - 1][x] - dc) <= A.grad_depth && fabsf(sD[y + 1][x] - dc) <= A.grad_depth;
    float4 rec;
    rec.x = Ic >= 0.0f ? Ic : 0.0f;
    rec.y = ok ? (Ir - Il) * 0.5f : 0.0f;
    rec.z = ok ? (Id - Iu) * 0.5f : 0.0f;
    rec.w = ok ? 1.0f : 0.0f;
    A.maps[g] = rec;
}

struct AssocArgs {
    const float *D;           // level depth [h_l, w_l]
    const float *I;           // level intensity [h_l, w_l]
    const float *mdepth;      // model depth [h_l, w_l]
    const float *mnormal;     // model normals [h_l, w_l, 3]
    const float4 *mmap;       // model map [h_l, w_l]
    const double *pose;       // current pose f64[12]
    const int *status;
    double *rows;             // [blocks, 29]
    float *jr, *pjr;          // [h_l*w_l, 7] or NULL: the geometric and the (unscaled) photometric row
    uint8_t *reason, *preason;  // [h_l*w_l] or NULL
    LevelCamera cam;
    float lambda, photo_thr;
};

__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, float ax, float ay)
{
    const float top = v00 + ax * (v01 - v00);
    const float bot = v10 + ax * (v11 - v10);
    return top + ay * (bot - top);
}

// The two reason codes of pixel `pix`; J / res are set when why == 0, pJ / pres (unscaled) when pwhy == 0.
__device__ void associate_pixel(const AssocArgs &A, const float R[9], const float t[3], int pix, int &why, float J[6],
                                float &res, int &pwhy, float pJ[6], float &pres)
{
    const bool photo = A.lambda != 0.0f;
    const LevelCamera &C = A.cam;
    const int r = pix / C.w, c = pix % C.w;
    const bool edge = r + 1 >= C.h || c + 1 >= C.w;
    // the live loads, together
    const float D = A.D[pix];
    const float Dd = edge ? 0.0f : A.D[pix + C.w], Dr = edge ? 0.0f : A.D[pix + 1];
    const float Il = A.I[pix];
    if (D == 0.0f) {
        why = 1;
        pwhy = photo ? 1 : 10;
        return;
    }
    float v[3];
    vertex(C, r, c, D, v);
    float n[3] = {0.0f, 0.0f, 0.0f};
    const bool normal_ok = Dd != 0.0f && Dr != 0.0f && live_normal(C, r, c, v, Dd, Dr, n);
    float p[3], nw[3], q[3];
    pose_transform(C, R, t, v, n, p, nw, q);
    float ux = 0.0f, uy = 0.0f, fc = 0.0f, fr = 0.0f;
    int stop = project(C, q, ux, uy, fc, fr);
    if (stop) {
        why = normal_ok ? stop : 2;
        pwhy = photo ? stop : 10;
        return;
    }
    // the model loads, together: depth, normal and the four records of the bilinear fetch hang on (ux, uy) alone
    const int mc = (int)fc, mr = (int)fr;
    const int mp = mr * C.w + mc;
    const float x0f = floorf(ux), y0f = floorf(uy);  // in [-1, w_l - 1] and [-1, h_l - 1] here
    const bool inside = x0f >= 0.0f && x0f <= (float)(C.w - 2) && y0f >= 0.0f && y0f <= (float)(C.h - 2);
    const int x0 = inside ? (int)x0f : 0, y0 = inside ? (int)y0f : 0;
    const int i00 = y0 * C.w + x0;
    const int right = C.w > 1 ? 1 : 0, down = C.h > 1 ? C.w : 0;
    const float dm = A.mdepth[mp];
    const float nm[3] = {A.mnormal[3 * (size_t)mp], A.mnormal[3 * (size_t)mp + 1], A.mnormal[3 * (size_t)mp + 2]};
    float4 c00 = {0, 0, 0, 0}, c01 = c00, c10 = c00, c11 = c00;
    if (photo) {
        c00 = A.mmap[i00];
        c01 = A.mmap[i00 + right];
        c10 = A.mmap[i00 + down];
        c11 = A.mmap[i00 + down + right];
    }
    float g[3];
    if (dm == 0.0f) {
        stop = 5;
    } else if (!model_gap(C, p, mr, mc, dm, g)) {
        stop = 6;
    } else if (!normal_ok) {
        why = 2;
    } else if (!normals_agree(C, nw, nm)) {
        why = 7;
    } else {
        why = 0;
        plane_row(p, nm, g, J, res);
    }
    if (stop) {
        why = normal_ok ? stop : 2;
        pwhy = photo ? stop : 10;
        return;
    }
    if (!photo) {
        pwhy = 10;
        return;
    }
    if (!(inside && c00.w != 0.0f && c01.w != 0.0f && c10.w != 0.0f && c11.w != 0.0f)) {
        pwhy = 8;
        return;
    }
    const float ax = ux - x0f, ay = uy - y0f;
    const float Im = lerp2(c00.x, c01.x, c10.x, c11.x, ax, ay);
    const float gx = lerp2(c00.y, c01.y, c10.y, c11.y, ax, ay);
    const float gy = lerp2(c00.z, c01.z, c10.z, c11.z, ax, ay);
    const float rI = Im - Il;
    if (!(fabsf(rI) <= A.photo_thr)) {
        pwhy = 9;
        return;
    }
    const float a0 = C.fx * gx, a1 = C.fy * gy;
    const float gc[3] = {a0 / q[2], a1 / q[2], -((a0 * q[0] + a1 * q[1]) / (q[2] * q[2]))};
    float a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = C.Rr[3 * i] * gc[0] + C.Rr[3 * i + 1] * gc[1] + C.Rr[3 * i + 2] * gc[2];
    pwhy = 0;
    pres = rI;
    pJ[0] = p[1] * a[2] - p[2] * a[1];
    pJ[1] = p[2] * a[0] - p[0] * a[2];
    pJ[2] = p[0] * a[1] - p[1] * a[0];
    pJ[3] = a[0];
    pJ[4] = a[1];
    pJ[5] = a[2];
}

__global__ __launch_bounds__(kTrackThreads) void track_rgbd_associate_kernel(AssocArgs A)
{
    if (A.status[0] != 0) return;  // a failed step froze the pose: nothing more to do (uniform over the grid)
    float R[9], t[3];
    load_pose_f32(A.pose, R, t);
    double acc[kTrackTerms];
#pragma unroll
    for (int e = 0; e < kTrackTerms; ++e) acc[e] = 0.0;
    for (int k = 0; k < kTrackPixPerThread; ++k) {
        const int pix = (int)blockIdx.x * kTrackPixPerBlock + k * kTrackThreads + (int)threadIdx.x;
        if (pix >= A.cam.npix) break;
        float J[6] = {0, 0, 0, 0, 0, 0}, res = 0.0f, pJ[6] = {0, 0, 0, 0, 0, 0}, pres = 0.0f;
        int why = 0, pwhy = 0;
        associate_pixel(A, R, t, pix, why, J, res, pwhy, pJ, pres);
        export_row(A.reason, A.jr, pix, why, J, res);
        export_row(A.preason, A.pjr, pix, pwhy, pJ, pres);
        if (!why) add_terms(acc, J, res);
        if (!pwhy) {
            float sJ[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) sJ[i] = A.lambda * pJ[i];
            add_terms(acc, sJ, A.lambda * pres);
            if (!why) acc[28] -= 1.0;  // the pixel counts once
        }
    }
    block_terms_to_row(acc, A.rows + (size_t)blockIdx.x * kTrackTerms);
}

static size_t maps_bytes(int h, int w, int levels) { return align256(total_pixels(h, w, levels) * sizeof(float4)); }

// depth pyramid | intensity pyramid | model maps | block rows | 256 bytes (the probe's stats row)
static size_t workspace_bytes(int h, int w, int levels)
{
    return 2 * pyramid_bytes(h, w, levels) + maps_bytes(h, w, levels) + rows_bytes(h, w);
}

static double *rows_of(void *ws, int h, int w, int levels)
{
    return (double *)((char *)ws + 2 * pyramid_bytes(h, w, levels) + maps_bytes(h, w, levels));
}

static int check_thresholds(const char *who, double dist, double angle, double delta, double frac, double weight,
                            double photo, double grad)
{
    if (!thresholds_in_range(dist, angle, delta, frac) || !(photo >= 0.0) || !isfinite(photo) || !(grad > 0.0) || !isfinite(grad))
        return fail(std::string(who) + ": thresholds out of range");
    if (!(weight >= 0.0) || !isfinite(weight)) return fail(std::string(who) + ": photo_weight must be finite and >= 0");
    return 0;
}

static void fill_prepare(PrepArgs &P, const float *depth, const uint8_t *mask, const uint8_t *image, void *ws, int h, int w,
                         int levels, double delta, double grad, double *pose, int *status, const double *init)
{
    P.depth = depth; P.mask = mask; P.image = (const uint32_t *)image;
    P.dpyr = (float *)ws;
    P.ipyr = (float *)((char *)ws + pyramid_bytes(h, w, levels));
    P.maps = (float4 *)((char *)ws + 2 * pyramid_bytes(h, w, levels));
    P.h = h; P.w = w; P.levels = levels;
    int off = 0, tile = 0;
    for (int l = 0; l <= OJF_TRACK_MAX_LEVELS; ++l) {
        P.off[l] = off;
        P.tile0[l] = tile;
        if (l < OJF_TRACK_MAX_LEVELS) P.mdepth[l] = nullptr, P.mcolor[l] = nullptr;
        if (l < levels) {
            off += (h >> l) * (w >> l);
            tile += (((h >> l) + kTileH - 1) / kTileH) * (((w >> l) + kTileW - 1) / kTileW);
        }
    }
    P.delta = (float)delta;
    P.grad_depth = (float)grad;
    P.pose = pose; P.status = status;
    for (int i = 0; i < 12; ++i) P.init[i] = init[i];
}

static void fill_assoc(AssocArgs &A, const PrepArgs &P, int l, const double *K, const float *Ki, const float *mdepth,
                       const float *mnormal, const double *Eref, double dist, double angle, double weight, double photo,
                       double *pose, const int *status, double *rows)
{
    A.D = P.dpyr + P.off[l];
    A.I = P.ipyr + P.off[l];
    A.mmap = P.maps + P.off[l];
    A.mdepth = mdepth; A.mnormal = mnormal; A.pose = pose; A.status = status; A.rows = rows;
    A.jr = A.pjr = nullptr; A.reason = A.preason = nullptr;
    fill_camera(A.cam, P.h, P.w, l, K, Ki, Eref, dist, angle);
    A.lambda = (float)weight;
    A.photo_thr = (float)photo;
}

static int launch_prepare(const PrepArgs &P, hipStream_t s)
{
    hipLaunchKernelGGL(track_rgbd_prepare_kernel, dim3(P.tile0[P.levels]), dim3(kTileW * kTileH), 0, s, P);
    OJF_HIP(hipGetLastError());
    return 0;
}

static int launch_associate(const AssocArgs &A, int blocks, hipStream_t s)
{
    hipLaunchKernelGGL(track_rgbd_associate_kernel, dim3(blocks), dim3(kTrackThreads), 0, s, A);
    OJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace rgbd
}  // namespace ojf

OJF_API size_t ojf_track_rgbd_workspace_bytes(int h, int w, int levels)
{
    using namespace ojf;
    return sizable(h, w, levels) ? rgbd::workspace_bytes(h, w, levels) : 0;
}

OJF_API int ojf_track_rgbd(const float *depth_dev, const uint8_t *mask_dev, const uint8_t *image_dev, int h, int w,
                           int levels, const double *K_host, const float *Kinv_host, const float *const *model_depth_host,
                           const float *const *model_normals_host, const uint8_t *const *model_color_host,
                           const double *E_ref_host, const double *E_init_host, const int *iterations_host,
                           double dist_thresh, double angle_thresh_deg, double pyramid_delta, double min_inlier_fraction,
                           double photo_weight, double photo_thresh, double grad_depth_limit, void *workspace_dev,
                           size_t workspace_bytes_, double *pose_dev, double *stats_dev, int *status_dev,
                           ojf_stream_t stream)
{
    using namespace ojf;
    using namespace ojf::rgbd;
    if (!depth_dev || !image_dev || !K_host || !Kinv_host || !model_depth_host || !model_normals_host || !model_color_host ||
        !E_ref_host || !E_init_host || !iterations_host || !workspace_dev || !pose_dev || !stats_dev || !status_dev)
        return fail("ojf_track_rgbd: null pointer argument");
    if (int rc = check_shape("ojf_track_rgbd", h, w, levels)) return rc;
    if (int rc = check_schedule("ojf_track_rgbd", levels, iterations_host, model_depth_host, model_normals_host,
                                model_color_host))
        return rc;
    if (int rc = check_thresholds("ojf_track_rgbd", dist_thresh, angle_thresh_deg, pyramid_delta, min_inlier_fraction,
                                  photo_weight, photo_thresh, grad_depth_limit))
        return rc;
    if (workspace_bytes_ < workspace_bytes(h, w, levels)) return fail("ojf_track_rgbd: workspace too small");
    const hipStream_t s = as_stream(stream);
    PrepArgs P;
    fill_prepare(P, depth_dev, mask_dev, image_dev, workspace_dev, h, w, levels, pyramid_delta, grad_depth_limit, pose_dev,
                 status_dev, E_init_host);
    double *rows = rows_of(workspace_dev, h, w, levels);
    AssocArgs A[OJF_TRACK_MAX_LEVELS];
    for (int l = 0; l < levels; ++l) {
        P.mdepth[l] = model_depth_host[l];
        P.mcolor[l] = (const uint32_t *)model_color_host[l];
        fill_assoc(A[l], P, l, K_host, Kinv_host + 9 * l, model_depth_host[l], model_normals_host[l], E_ref_host, dist_thresh,
                   angle_thresh_deg, photo_weight, photo_thresh, pose_dev, status_dev, rows);
    }
    if (int rc = launch_prepare(P, s)) return rc;
    return run_steps(h, w, levels, iterations_host, min_inlier_fraction, rows, pose_dev, status_dev, stats_dev, nullptr,
                     E_init_host, s, [&](int l, int blocks) { return launch_associate(A[l], blocks, s); });
}

OJF_API int ojf_track_rgbd_associate(const float *depth_dev, const uint8_t *mask_dev, const uint8_t *image_dev, int h, int w,
                                     int level, const double *K_host, const float *Kinv_host, const float *model_depth_dev,
                                     const float *model_normals_dev, const uint8_t *model_color_dev,
                                     const double *E_ref_host, const double *E_pose_host, double dist_thresh,
                                     double angle_thresh_deg, double pyramid_delta, double min_inlier_fraction,
                                     double photo_weight, double photo_thresh, double grad_depth_limit, void *workspace_dev,
                                     size_t workspace_bytes_, double *pose_dev, double *sums_dev, float *jr_dev,
                                     uint8_t *reason_dev, float *photo_jr_dev, uint8_t *photo_reason_dev, int *status_dev,
                                     ojf_stream_t stream)
{
    using namespace ojf;
    using namespace ojf::rgbd;
    if (!depth_dev || !image_dev || !K_host || !Kinv_host || !model_depth_dev || !model_normals_dev || !model_color_dev ||
        !E_ref_host || !E_pose_host || !workspace_dev || !pose_dev || !sums_dev || !status_dev)
        return fail("ojf_track_rgbd_associate: null pointer argument");
    if (level < 0) return fail("ojf_track_rgbd_associate: levels must be 1..OJF_TRACK_MAX_LEVELS");
    const int levels = level + 1;
    if (int rc = check_shape("ojf_track_rgbd_associate", h, w, levels)) return rc;
    if (int rc = check_thresholds("ojf_track_rgbd_associate", dist_thresh, angle_thresh_deg, pyramid_delta,
                                  min_inlier_fraction, photo_weight, photo_thresh, grad_depth_limit))
        return rc;
    if (workspace_bytes_ < workspace_bytes(h, w, levels)) return fail("ojf_track_rgbd_associate: workspace too small");
    const hipStream_t s = as_stream(stream);
    PrepArgs P;
    fill_prepare(P, depth_dev, mask_dev, image_dev, workspace_dev, h, w, levels, pyramid_delta, grad_depth_limit, pose_dev,
                 status_dev, E_pose_host);
    P.mdepth[level] = model_depth_dev;
    P.mcolor[level] = (const uint32_t *)model_color_dev;
    double *rows = rows_of(workspace_dev, h, w, levels);
    double *stats = (double *)((char *)workspace_dev + workspace_bytes(h, w, levels) - 256);  // the stats row goes to the scratch tail
    AssocArgs A;
    fill_assoc(A, P, level, K_host, Kinv_host, model_depth_dev, model_normals_dev, E_ref_host, dist_thresh, angle_thresh_deg,
               photo_weight, photo_thresh, pose_dev, status_dev, rows);
    A.jr = jr_dev;
    A.reason = reason_dev;
    A.pjr = photo_jr_dev;
    A.preason = photo_reason_dev;
    int one_step[OJF_TRACK_MAX_LEVELS] = {};
    one_step[level] = 1;
    if (int rc = launch_prepare(P, s)) return rc;
    return run_steps(h, w, levels, one_step, min_inlier_fraction, rows, pose_dev, status_dev, stats, sums_dev, E_pose_host, s,
                     [&](int, int blocks) { return launch_associate(A, blocks, s); });
}
