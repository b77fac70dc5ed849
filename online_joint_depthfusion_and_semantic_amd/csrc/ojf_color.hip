// COLOR: a colour volume beside the fused geometry (KinectFusion's colour volume / InfiniTAM / Open3D style) - fusion of
// n colour views by the voxel-projective sweep of ojf_projective.hip, and its trilinear read-out at points and at the hit
// points of a rendered depth image.  Own definition (the reference has no counterpart); tests/color_ref.py restates it in
// numpy and the GPU tests pin the kernels to it bit for bit.
//
// The volume: fp16 [X,Y,Z,4], voxel-major, 8 B per voxel (c0, c1, c2, W): the running mean of the three image channels on
// the image's own 0..255 scale, in the order the image brings them, and the colour weight W; W == 0: no colour yet; all
// zeros at reset.  (fp16, not u8: see DESIGN.md 11.)  The frame is the one of extract / integrate / render / projective:
// voxel (i,j,k) has its centre at origin + (i+0.5, j+0.5, k+0.5)·res.
//
// Normative definition.  All device arithmetic is fp32 with every product, sum and division rounded on its own (the
// build's -ffp-contract=off and correctly rounded division); fp16 conversions round to nearest even; max / min are IEEE
// maxNum / minNum.
//
// ojf_fuse_color, per voxel (i,j,k), for views v = 0..n-1 in that order ("skip": this view leaves the voxel alone):
//     1. steps 1-3 of ojf_fuse_projective exactly (ojf_projview.h: the same host f64 constants A, b, fx, fy, cx, cy, the
//        same projection, nearest pixel floor(u + 0.5), float bounds checks, depth and mask tests) give the pixel px and
//        its depth d, and zc.
//     2. s = d - zc;  skip unless -band <= s <= band (colour is written near the observed surface only; no carving).
//     3. w0 = float(W), w1 = w0 + 1;  for k = 0, 1, 2:  c_k = half((w0·float(c_k) + float(image[px][k])) / w1).
//     4. W = half(min(w1, max_weight)).
//   band > 0 finite; 1 <= max_weight <= 2048; near >= 0.  The TSDF and weight volumes are never read.
//
// Sample S(g), g in voxel index coordinates (voxel (i,j,k) sits at g = (i,j,k)), N = (X, Y, Z):
//     (0,0,0,0) if any g_a is non-finite, < -1 or > N_a (float comparisons, before any conversion to int).  Else
//     i0_a = floor(g_a), f_a = g_a - i0_a; over the corners 000..111 (bits x, y, z), a corner counts only if it lies inside
//     the grid and has float(W) > 0: tw = (wx·wy)·wz with w_axis = (1 - f) or f;  acc_k = acc_k + tw·float(c_k),
//     ws = ws + tw (both from 0).  ws > 0: out_k = u8(floor(min(max(acc_k / ws, 0), 255) + 0.5)), alpha = 255; else all four
//     bytes 0.  Unobserved neighbours do not darken a colour.
// ojf_color_sample: rgba[i] = S(points[i]).
// ojf_color_render: per pixel (r, c) of view v with t = depth[v][r][c]: 0 unless t is finite and > 0; else, with o, dc, d,
//     dv exactly as the header of ojf_render.hip defines the ray, p_i = o_i + t·dv_i, g_i = p_i - 0.5, rgba = S(g).  (The
//     depth image ojf_render produced reproduces its hit point p*.)
//
// Shape.  Fusion: every voxel is owned by one lane for the whole call; a lane owns 4 consecutive voxels of the flattened
// volume (32 B: two 16-byte accesses; lanes run along the contiguous z axis) and walks the n views in order with the
// voxels' fp16 bits in registers.  The loads are issued lazily, once some voxel of the group has a view that reaches
// step 3, and a group is stored only if it was loaded: a sweep touches the volume only where the views see a surface.
// The image gather is one 32-bit load per (voxel, view).  Values are rounded to fp16 after every view, so n views in one
// call give the bits of n calls of one view.  No atomics, no LDS, no workspace.  The last group of a volume whose voxel
// count is no multiple of 4, and every group of a volume whose pointer is not 16-byte aligned, go element by element.
// Read-out: one lane per output, every output written once; the 8 corners are 8-byte loads (2-byte loads for a volume
// off the 8-byte grid).
#include "ojf_projview.h"
#include "ojf_renderview.h"

namespace ojf {

constexpr int kColorGroup = 4;
constexpr int kColorBlock = 256;
constexpr int kColorRenderViewsPerLaunch = 32;  // keeps the by-value views well inside the kernel-argument segment

struct ColorArgs {
    uint16_t *color;
    ProjImages im;
    const uint32_t *image;  // u8[n,h,w,4] read as one word per pixel (byte k: channel k)
    uint32_t total, groups;
    int Y, Z, n, vec;
    float band, max_weight;
};

struct ColorLaunch {
    ColorArgs a;
    ProjView v[OJF_COLOR_MAX_VIEWS];
};

__global__ __launch_bounds__(kColorBlock) void color_kernel(ColorLaunch L)
{
    const ColorArgs &P = L.a;
    const uint32_t g = blockIdx.x * kColorBlock + threadIdx.x;
    if (g >= P.groups) return;
    const uint32_t first = g * kColorGroup;
    const int cnt = P.total - first < (uint32_t)kColorGroup ? (int)(P.total - first) : kColorGroup;
    const bool vec = P.vec && cnt == kColorGroup;

    float xs[kColorGroup], ys[kColorGroup], zs[kColorGroup];
    voxel_indices<kColorGroup>(first, P.Y, P.Z, xs, ys, zs);

    uint32_t q[2 * kColorGroup];  // voxel e: q[2e] = c0 | c1 << 16, q[2e+1] = c2 | W << 16
#pragma unroll
    for (int i = 0; i < 2 * kColorGroup; ++i) q[i] = 0;
    uint16_t *const vox = P.color + 4 * (size_t)first;
    bool loaded = false;

    for (int v = 0; v < P.n; ++v) {
        const ProjView &V = L.v[v];
        uint32_t rgb[kColorGroup];
        uint32_t hit = 0;
#pragma unroll
        for (int e = 0; e < kColorGroup; ++e) {
            rgb[e] = 0;
            if (e >= cnt) continue;
            uint32_t px;
            float s;
            if (!project_depth(V, P.im, v, xs[e], ys[e], zs[e], px, s)) continue;
            if (!(s >= -P.band && s <= P.band)) continue;
            rgb[e] = P.image[px];
            hit |= 1u << e;
        }
        if (!hit) continue;
        if (!loaded) {
            if (vec) {
#pragma unroll
                for (int i = 0; i < kColorGroup / 2; ++i) {
                    const uint4 r = reinterpret_cast<const uint4 *>(vox)[i];
                    q[4 * i] = r.x; q[4 * i + 1] = r.y; q[4 * i + 2] = r.z; q[4 * i + 3] = r.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4 * kColorGroup; ++i)
                    if (i < 4 * cnt) set16(q, i, vox[i]);
            }
            loaded = true;
        }
#pragma unroll
        for (int e = 0; e < kColorGroup; ++e) {
            if (!((hit >> e) & 1u)) continue;
            const float w0 = h2f((uint16_t)get16(q, 4 * e + 3));
            const float w1 = w0 + 1.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float c0 = h2f((uint16_t)get16(q, 4 * e + k));
                const float x = (float)((rgb[e] >> (8 * k)) & 0xffu);
                set16(q, 4 * e + k, f2h((w0 * c0 + x) / w1));
            }
            set16(q, 4 * e + 3, f2h(fminf(w1, P.max_weight)));
        }
    }

    if (!loaded) return;
    if (vec) {
#pragma unroll
        for (int i = 0; i < kColorGroup / 2; ++i)
            reinterpret_cast<uint4 *>(vox)[i] = make_uint4(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4 * kColorGroup; ++i)
            if (i < 4 * cnt) vox[i] = (uint16_t)get16(q, i);
    }
}

// ---- read-out ----------------------------------------------------------------------------------------------------------
struct ColorVolume {
    const uint16_t *color;
    int X, Y, Z, al8;  // al8: the pointer is 8-byte aligned (one load per voxel)
};

// S(g) of the definition, as the word c0 | c1 << 8 | c2 << 16 | alpha << 24 (the four bytes in memory order)
__device__ __forceinline__ uint32_t sample_color(const ColorVolume &C, const float g[3])
{
    const int N[3] = {C.X, C.Y, C.Z};
    int i0[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(g[a] >= -1.0f && g[a] <= (float)N[a])) return 0;  // (a NaN or inf fails)
        const float fl = floorf(g[a]);
        f[a] = g[a] - fl;
        i0[a] = (int)fl;
    }
    float acc[3] = {0.0f, 0.0f, 0.0f}, ws = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int bi = (c >> 2) & 1, bj = (c >> 1) & 1, bk = c & 1;
        const int i = i0[0] + bi, j = i0[1] + bj, k = i0[2] + bk;
        if (i < 0 || i >= C.X || j < 0 || j >= C.Y || k < 0 || k >= C.Z) continue;
        const uint16_t *p = C.color + 4 * (((size_t)i * C.Y + j) * C.Z + k);
        uint32_t lo, hi;
        if (C.al8) {
            const uint2 r = *reinterpret_cast<const uint2 *>(p);
            lo = r.x; hi = r.y;
        } else {
            lo = p[0] | ((uint32_t)p[1] << 16);
            hi = p[2] | ((uint32_t)p[3] << 16);
        }
        if (!(h2f((uint16_t)(hi >> 16)) > 0.0f)) continue;
        const float wx = bi ? f[0] : 1.0f - f[0];
        const float wy = bj ? f[1] : 1.0f - f[1];
        const float wz = bk ? f[2] : 1.0f - f[2];
        const float tw = (wx * wy) * wz;
        acc[0] = acc[0] + tw * h2f((uint16_t)(lo & 0xffffu));
        acc[1] = acc[1] + tw * h2f((uint16_t)(lo >> 16));
        acc[2] = acc[2] + tw * h2f((uint16_t)(hi & 0xffffu));
        ws = ws + tw;
    }
    if (!(ws > 0.0f)) return 0;
    uint32_t out = 0xff000000u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float m = floorf(fminf(fmaxf(acc[k] / ws, 0.0f), 255.0f) + 0.5f);
        out |= (uint32_t)(int)m << (8 * k);
    }
    return out;
}

__global__ __launch_bounds__(kColorBlock) void color_sample_kernel(ColorVolume C, const float *points, uint32_t n, uint32_t *rgba)
{
    const uint32_t i = blockIdx.x * kColorBlock + threadIdx.x;
    if (i >= n) return;
    const float g[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
    rgba[i] = sample_color(C, g);
}

struct ColorRenderLaunch {
    ColorVolume C;
    const float *depth;  // of the launch's first view
    uint32_t *rgba;
    int h, w;
    float res;
    RenderView v[kColorRenderViewsPerLaunch];
};

__global__ __launch_bounds__(kColorBlock) void color_render_kernel(ColorRenderLaunch L)
{
    const uint32_t i = blockIdx.x * kColorBlock + threadIdx.x;  // pixel of view blockIdx.y
    if (i >= (uint32_t)(L.h * L.w)) return;
    const RenderView &V = L.v[blockIdx.y];
    const size_t pix = (size_t)blockIdx.y * (size_t)(L.h * L.w) + i;
    const float t = L.depth[pix];
    uint32_t out = 0;
    if (fabsf(t) < INFINITY && t > 0.0f) {
        const float cf = (float)(i % (uint32_t)L.w), rf = (float)(i / (uint32_t)L.w);
        float dc[3], g[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) dc[a] = V.Ki[3 * a] * cf + V.Ki[3 * a + 1] * rf + V.Ki[3 * a + 2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float d = V.R[3 * a] * dc[0] + V.R[3 * a + 1] * dc[1] + V.R[3 * a + 2] * dc[2];
            const float dv = d / L.res;
            const float p = V.o[a] + t * dv;
            g[a] = p - 0.5f;
        }
        out = sample_color(L.C, g);
    }
    L.rgba[pix] = out;
}

}  // namespace ojf

OJF_API int ojf_fuse_color(uint16_t *color, int X, int Y, int Z, const double *origin, double res, int n, const double *K,
                           const double *E, const float *depth, const uint8_t *mask, const uint8_t *image, int h, int w,
                           float band, float max_weight, float near, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_fuse_color";
    if (!color || !origin || !K || !E || !depth || !image) return refuse(who, "null pointer argument");
    if (!(band > 0.0f) || !std::isfinite(band)) return refuse(who, "band must be > 0 and finite");
    if (int rc = check_projective_views(who, X, Y, Z, origin, res, n, OJF_COLOR_MAX_VIEWS, K, E, h, w, max_weight, near)) return rc;
    if (((uintptr_t)color & 1) || ((uintptr_t)image & 3)) return refuse(who, "color_dev must be 2-byte and image_dev 4-byte aligned");
    ColorLaunch L;
    ColorArgs &A = L.a;
    A.color = color;
    fill_proj_images(A.im, depth, mask, h, w, near);
    A.image = reinterpret_cast<const uint32_t *>(image);
    A.total = (uint32_t)((int64_t)X * Y * Z);
    A.groups = (A.total + kColorGroup - 1) / kColorGroup;
    A.Y = Y; A.Z = Z; A.n = n;
    A.vec = ((uintptr_t)color & 15) == 0;  // anything else goes element by element
    A.band = band; A.max_weight = max_weight;
    make_proj_views(K, E, origin, res, n, L.v);
    const uint32_t blocks = (A.groups + kColorBlock - 1) / kColorBlock;
    hipLaunchKernelGGL(color_kernel, dim3(blocks), dim3(kColorBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_color_sample(const uint16_t *color, int X, int Y, int Z, const float *points, size_t n, uint8_t *rgba,
                             ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_color_sample";
    if (!color || !points || !rgba) return refuse(who, "null pointer argument");
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    if (n < 1 || n > 0x7fffffffULL) return refuse(who, "n must be 1..2^31-1 points");
    if (((uintptr_t)color & 1) || ((uintptr_t)points & 3) || ((uintptr_t)rgba & 3))
        return refuse(who, "color_dev must be 2-byte, points_dev and rgba_dev 4-byte aligned");
    const ColorVolume C{color, X, Y, Z, ((uintptr_t)color & 7) == 0};
    const uint32_t blocks = ((uint32_t)n + kColorBlock - 1) / kColorBlock;
    hipLaunchKernelGGL(color_sample_kernel, dim3(blocks), dim3(kColorBlock), 0, as_stream(stream), C, points, (uint32_t)n,
                       reinterpret_cast<uint32_t *>(rgba));
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_color_render(const uint16_t *color, int X, int Y, int Z, const double *origin, double res, int n,
                             const float *Kinv, const float *E, const float *depth, int h, int w, uint8_t *rgba,
                             ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_color_render";
    if (!color || !origin || !Kinv || !E || !depth || !rgba) return refuse(who, "null pointer argument");
    if (n < 1 || n > OJF_RENDER_MAX_VIEWS) return refuse(who, "n must be 1..OJF_RENDER_MAX_VIEWS views");
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    if (h <= 0 || w <= 0) return refuse(who, "non-positive image size");
    if ((int64_t)n * h * w > 0x7fffffffLL) return refuse(who, "images too large");
    bool finite = all_finite(origin, 3) && std::isfinite(res);
    for (int i = 0; i < 9 * n; ++i) finite &= std::isfinite(Kinv[i]);
    for (int i = 0; i < 12 * n; ++i) finite &= std::isfinite(E[i]);
    if (!finite) return refuse(who, "non-finite Kinv, E, origin or resolution");
    if (!(res > 0.0)) return refuse(who, "resolution must be > 0");
    if (((uintptr_t)color & 1) || ((uintptr_t)rgba & 3)) return refuse(who, "color_dev must be 2-byte and rgba_dev 4-byte aligned");
    ColorRenderLaunch L;
    L.C = ColorVolume{color, X, Y, Z, ((uintptr_t)color & 7) == 0};
    L.h = h; L.w = w;
    L.res = (float)res;
    const uint32_t blocks = ((uint32_t)(h * w) + kColorBlock - 1) / kColorBlock;
    for (int v0 = 0; v0 < n; v0 += kColorRenderViewsPerLaunch) {
        const int nv = n - v0 < kColorRenderViewsPerLaunch ? n - v0 : kColorRenderViewsPerLaunch;
        L.depth = depth + (size_t)v0 * h * w;
        L.rgba = reinterpret_cast<uint32_t *>(rgba) + (size_t)v0 * h * w;
        for (int j = 0; j < nv; ++j) make_render_view(Kinv + 9 * (v0 + j), E + 12 * (v0 + j), origin, res, L.v[j]);
        hipLaunchKernelGGL(color_render_kernel, dim3(blocks, nv), dim3(kColorBlock), 0, as_stream(stream), L);
        OJF_HIP(hipGetLastError());
    }
    return 0;
}
