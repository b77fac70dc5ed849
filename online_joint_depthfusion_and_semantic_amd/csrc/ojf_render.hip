// RENDER: ray casting of depth, normal and label images from a fused fp16 TSDF volume (KinectFusion-style), n views of one
// volume per call.  Own definition (the reference has only an offline CPU ray caster that looks for an occupancy value,
// not a zero crossing); tests/render_ref.py restates it in fp32 numpy and the GPU tests pin the kernel to it bit for bit.
//
// Normative definition.  All arithmetic is fp32 with every product, sum, division and sqrt rounded on its own (the build's
// -ffp-contract=off, correctly rounded division and sqrt); "a + b + c" below means (a + b) + c.  N = (X, Y, Z).
//   Volume frame: voxel (i,j,k) has its centre at origin + (i+0.5, j+0.5, k+0.5)·res (the frame of extract / integrate,
//     ojf_common.h ray_sample; NOT the mesh frame of get_mesh).  Voxel coordinates p = (x - origin) / res.
//   Per view (host, f64): o = fp32((E[:,3] - origin) / res); resf = fp32(res).
//   Ray of pixel (r, c):  dc_i = Ki[3i]·c + Ki[3i+1]·r + Ki[3i+2]          (integer pixel coordinates, z = 1)
//                         d_i  = E[4i]·dc_0 + E[4i+1]·dc_1 + E[4i+2]·dc_2
//                         dv_i = d_i / resf;  len = sqrt(d_0·d_0 + d_1·d_1 + d_2·d_2)
//     The point of parameter t is o + t·dv (voxel units); since dc_2 = 1, t is the camera z-depth.
//   Range (slab test against the trilinear support box [0.5, N-0.5] on every axis): t0 = -inf, t1 = +inf; per axis with
//     dv_i != 0: ta = (0.5 - o_i) / dv_i, tb = ((N_i - 0.5) - o_i) / dv_i, t0 = max(t0, min(ta, tb)), t1 = min(t1, max(ta, tb));
//     an axis with dv_i == 0 and o_i outside [0.5, N_i - 0.5] makes the pixel a miss.  Then t0 = max(t0, near); the
//     pixel is a miss unless t0 <= t1.
//   Sample F(p) at voxel point p: q_i = p_i - 0.5, fl_i = min(max(floor(q_i), 0), N_i - 2), a_i = q_i - fl_i; over the
//     corners 000..111 (bits x, y, z) F = F + w·T[fl + corner] from F = 0, w = wx·wy·wz with w_axis = (1 - a) or a.
//     Valid: no weight volume, or all 8 corner weights > 0.  March samples take p_i = o_i + t·dv_i.
//   March: t = t0; sample; then t = t + max(0.5·resf, 0.75·max(F, 0)) / len; while t <= t1, at most 2·(X+Y+Z) samples.
//     max() / min() are IEEE maxNum / minNum (a NaN operand yields the other one).
//   Hit: the first consecutive samples (k-1, k) that are both valid with F_{k-1} > 0 and F_k <= 0 (back faces are not
//     hits).  t* = t_{k-1} + ((t_k - t_{k-1})·F_{k-1}) / (F_{k-1} - F_k);  p* = o + t*·dv.
//     depth = t*;  label = ids at clamp(floor(p*), 0, N-1);
//     normal: g_a = F(p* + e_a) - F(p* - e_a) (the shifted coordinate is the fp32 p*_a ± 1), n = g / sqrt(g·g) (zero when
//     g·g == 0, or when any of the six points has a coordinate outside [0.5, N-0.5]); world frame, points to the free
//     (positive) side.
//   Miss: depth, normal and label are 0 (the datasets' "no depth").
// Validity is only needed at a candidate crossing: the kernel gathers the weights there (re-evaluating the previous
// sample's position from its t - the same bits), not at every sample.
//
// Shape: one lane per pixel, one 64-lane wave per 8x8 pixel tile (the rays of a wave gather the same cache lines of the
// z-contiguous volume), four tiles per block, blockIdx.y = view.  Blocks banded over the XCDs like extract.  The march
// loop is divergent per lane and ends for the wave when its last lane is done.  No LDS, no atomics, every output written
// once: the same bits on every run and for every n.
#include "ojf_renderview.h"

#include <math.h>

namespace ojf {

constexpr int kRenderTilesPerBlock = 4;
constexpr int kRenderViewsPerLaunch = 32;  // keeps the by-value views well inside the kernel-argument segment

struct RenderArgs {
    const uint16_t *tsdf;
    const uint16_t *wgt;  // NULL: every voxel observed
    const uint8_t *ids;   // NULL: no labels
    float *depth;         // [n, h, w]
    float *normals;       // [n, h, w, 3] or NULL
    uint8_t *labels;      // [n, h, w] or NULL
    int X, Y, Z, h, w, tiles_x, n_tiles, max_samples;
    float res, near;
    int view0;            // view index of blockIdx.y == 0 (launches of more than kRenderViewsPerLaunch views)
};

struct RenderLaunch {
    RenderArgs a;
    RenderView v[kRenderViewsPerLaunch];
};

// corner offsets and trilinear weights of the sample at voxel point p (the definition's q, fl, a)
struct Stencil {
    int base;
    float a[3];
};

__device__ __forceinline__ Stencil stencil(const float p[3], const RenderArgs &A)
{
    const int N[3] = {A.X, A.Y, A.Z};
    float fl[3];
    Stencil s;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float q = p[i] - 0.5f;
        fl[i] = fminf(fmaxf(floorf(q), 0.0f), (float)(N[i] - 2));
        s.a[i] = q - fl[i];
    }
    s.base = ((int)fl[0] * A.Y + (int)fl[1]) * A.Z + (int)fl[2];
    return s;
}

__device__ __forceinline__ float sample_tsdf(const float p[3], const RenderArgs &A)
{
    const Stencil s = stencil(p, A);
    const int yz = A.Y * A.Z;
    float F = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int bi = (c >> 2) & 1, bj = (c >> 1) & 1, bk = c & 1;
        const float wx = bi ? s.a[0] : 1.0f - s.a[0];
        const float wy = bj ? s.a[1] : 1.0f - s.a[1];
        const float wz = bk ? s.a[2] : 1.0f - s.a[2];
        const float wq = wx * wy * wz;
        F = F + wq * h2f(A.tsdf[s.base + bi * yz + bj * A.Z + bk]);
    }
    return F;
}

__device__ __forceinline__ bool sample_valid(const float p[3], const RenderArgs &A)
{
    if (!A.wgt) return true;
    const Stencil s = stencil(p, A);
    const int yz = A.Y * A.Z;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int bi = (c >> 2) & 1, bj = (c >> 1) & 1, bk = c & 1;
        ok &= h2f(A.wgt[s.base + bi * yz + bj * A.Z + bk]) > 0.0f;
    }
    return ok;
}

__device__ __forceinline__ void ray_point(const float o[3], const float dv[3], float t, float p[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = o[i] + t * dv[i];
}

__device__ __forceinline__ bool in_support(const float p[3], const RenderArgs &A)
{
    return p[0] >= 0.5f && p[0] <= (float)A.X - 0.5f && p[1] >= 0.5f && p[1] <= (float)A.Y - 0.5f && p[2] >= 0.5f &&
           p[2] <= (float)A.Z - 0.5f;
}

__global__ __launch_bounds__(64 * kRenderTilesPerBlock) void render_kernel(RenderLaunch L)
{
    const RenderArgs &A = L.a;
    const RenderView &V = L.v[blockIdx.y];
    const int tile = banded_block_x() * kRenderTilesPerBlock + (int)(threadIdx.x >> 6);
    if (tile >= A.n_tiles) return;
    const int lane = threadIdx.x & 63;
    const int r = (tile / A.tiles_x) * 8 + (lane >> 3);
    const int c = (tile % A.tiles_x) * 8 + (lane & 7);
    if (r >= A.h || c >= A.w) return;

    const float cf = (float)c, rf = (float)r;
    float dc[3], dv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) dc[i] = V.Ki[3 * i] * cf + V.Ki[3 * i + 1] * rf + V.Ki[3 * i + 2];
    float d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d[i] = V.R[3 * i] * dc[0] + V.R[3 * i + 1] * dc[1] + V.R[3 * i + 2] * dc[2];
        dv[i] = d[i] / A.res;
    }
    const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);

    // slab test
    const int N[3] = {A.X, A.Y, A.Z};
    float t0 = -INFINITY, t1 = INFINITY;
    bool miss = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float lo = 0.5f, hi = (float)N[i] - 0.5f;
        if (dv[i] != 0.0f) {
            const float ta = (lo - V.o[i]) / dv[i], tb = (hi - V.o[i]) / dv[i];
            t0 = fmaxf(t0, fminf(ta, tb));
            t1 = fminf(t1, fmaxf(ta, tb));
        } else if (V.o[i] < lo || V.o[i] > hi) {
            miss = true;
        }
    }
    t0 = fmaxf(t0, A.near);
    miss |= !(t0 <= t1);

    float depth = 0.0f, nrm[3] = {0.0f, 0.0f, 0.0f};
    uint8_t label = 0;
    if (!miss) {
        const float half = 0.5f * A.res;
        float t = t0, tp = 0.0f, Fp = 0.0f, F = 0.0f;
        bool hit = false;
        for (int k = 0; k < A.max_samples && t <= t1; ++k) {
            float p[3];
            ray_point(V.o, dv, t, p);
            F = sample_tsdf(p, A);
            if (k > 0 && Fp > 0.0f && F <= 0.0f) {
                float pp[3];
                ray_point(V.o, dv, tp, pp);
                if (sample_valid(pp, A) && sample_valid(p, A)) {
                    hit = true;
                    break;
                }
            }
            tp = t;
            Fp = F;
            t = t + fmaxf(half, 0.75f * fmaxf(F, 0.0f)) / len;
        }
        if (hit) {
            // (t, F) = sample k, (tp, Fp) = sample k-1
            depth = tp + ((t - tp) * Fp) / (Fp - F);
            float ps[3];
            ray_point(V.o, dv, depth, ps);
            if (A.ids) {
                int vi[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) vi[i] = (int)fminf(fmaxf(floorf(ps[i]), 0.0f), (float)(N[i] - 1));
                label = A.ids[(vi[0] * A.Y + vi[1]) * A.Z + vi[2]];
            }
            if (A.normals) {
                float g[3];
                bool inside = true;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    float pa[3] = {ps[0], ps[1], ps[2]}, pb[3] = {ps[0], ps[1], ps[2]};
                    pa[ax] = ps[ax] + 1.0f;
                    pb[ax] = ps[ax] - 1.0f;
                    inside &= in_support(pa, A) && in_support(pb, A);
                    g[ax] = inside ? sample_tsdf(pa, A) - sample_tsdf(pb, A) : 0.0f;
                }
                const float gg = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
                if (inside && gg > 0.0f) {
                    const float gl = sqrtf(gg);
#pragma unroll
                    for (int i = 0; i < 3; ++i) nrm[i] = g[i] / gl;
                }
            }
        }
    }
    const size_t pix = ((size_t)(A.view0 + blockIdx.y) * A.h + r) * A.w + c;
    A.depth[pix] = depth;
    if (A.normals) {
        A.normals[3 * pix + 0] = nrm[0];
        A.normals[3 * pix + 1] = nrm[1];
        A.normals[3 * pix + 2] = nrm[2];
    }
    if (A.labels) A.labels[pix] = label;
}

}  // namespace ojf

OJF_API int ojf_render(const uint16_t *tsdf, const uint16_t *wgt, const uint8_t *ids, int X, int Y, int Z,
                       const double *origin, double res, int n, const float *Kinv, const float *E, int h, int w,
                       float near, float *depth, float *normals, uint8_t *labels, ojf_stream_t stream)
{
    using namespace ojf;
    if (!tsdf || !depth || !origin || !Kinv || !E) return fail("ojf_render: null pointer argument");
    if (n < 1 || n > OJF_RENDER_MAX_VIEWS) return fail("ojf_render: n must be 1..OJF_RENDER_MAX_VIEWS views");
    if (X < 2 || Y < 2 || Z < 2) return fail("ojf_render: the volume needs at least 2 voxels per axis");
    if ((int64_t)X * Y * Z > 0x7fffffffLL) return fail("ojf_render: volume too large");
    if (h <= 0 || w <= 0) return fail("ojf_render: non-positive image size");
    if ((int64_t)n * h * w > 0x7fffffffLL) return fail("ojf_render: images too large");
    if (!(res > 0.0)) return fail("ojf_render: resolution must be > 0");
    if (labels && !ids) return fail("ojf_render: labels need an id volume");
    RenderLaunch L;
    RenderArgs &A = L.a;
    A.tsdf = tsdf; A.wgt = wgt; A.ids = ids; A.depth = depth; A.normals = normals; A.labels = labels;
    A.X = X; A.Y = Y; A.Z = Z; A.h = h; A.w = w;
    A.tiles_x = (w + 7) / 8;
    A.n_tiles = A.tiles_x * ((h + 7) / 8);
    A.max_samples = 2 * (X + Y + Z);
    A.res = (float)res;
    A.near = near;
    const int blocks = (A.n_tiles + kRenderTilesPerBlock - 1) / kRenderTilesPerBlock;
    for (int v0 = 0; v0 < n; v0 += kRenderViewsPerLaunch) {
        const int nv = n - v0 < kRenderViewsPerLaunch ? n - v0 : kRenderViewsPerLaunch;
        A.view0 = v0;
        for (int j = 0; j < nv; ++j) make_render_view(Kinv + 9 * (v0 + j), E + 12 * (v0 + j), origin, res, L.v[j]);
        hipLaunchKernelGGL(render_kernel, dim3((blocks + 7) / 8 * 8, nv), dim3(64 * kRenderTilesPerBlock), 0, as_stream(stream), L);
        OJF_HIP(hipGetLastError());
    }
    return 0;
}
