// What the voxel-projective sweeps (ojf_projective.hip, ojf_color.hip, ojf_labels.hip) share: the per-view constants the
// host prepares in f64 and steps 1-3 of the definition in ojf_projective.hip's header - voxel -> camera point -> nearest
// pixel -> depth and mask tests.  One text for all kernels, so that colour and label votes land in exactly the voxels the
// depth of the same frame reaches.  The operation order is normative (see there); nothing here may be re-associated.
// The packed lanes and the host checks of a box that the sweeps use are in ojf_blocks.h, shared with the other operators.
#pragma once
#include "ojf_blocks.h"

namespace ojf {

struct ProjView {  // 16 floats, by value in the kernel arguments
    float A[9];    // A[3a+m]
    float b[3];
    float fx, fy, cx, cy;
};

struct ProjImages {  // the depth images of a call and what bounds a projection into them
    const float *depth;
    const uint8_t *mask;
    int h, w;
    float near, cmax, rmax;  // cmax = w - 1, rmax = h - 1
};

// voxel indices, as floats, of `count` consecutive elements of the flattened [X,Y,Z] volume from `first` on (a group may
// run over the end of a z row)
template <int count>
__device__ __forceinline__ void voxel_indices(uint32_t first, int Y, int Z, float xs[count], float ys[count], float zs[count])
{
    uint32_t k = first % (uint32_t)Z;
    const uint32_t row = first / (uint32_t)Z;
    uint32_t j = row % (uint32_t)Y, i = row / (uint32_t)Y;
#pragma unroll
    for (int e = 0; e < count; ++e) {
        xs[e] = (float)i; ys[e] = (float)j; zs[e] = (float)k;
        if (++k == (uint32_t)Z) {
            k = 0;
            if (++j == (uint32_t)Y) { j = 0; ++i; }
        }
    }
}

// Steps 1-3 for voxel (x, y, z) and view v: false when the view leaves the voxel alone; else px = the pixel's index in
// [n,h,w] and s = d - zc.
__device__ __forceinline__ bool project_depth(const ProjView &V, const ProjImages &I, int v, float x, float y, float z,
                                              uint32_t &px, float &s)
{
    const float zc = ((V.A[6] * x + V.A[7] * y) + V.A[8] * z) + V.b[2];
    if (!(zc > I.near)) return false;
    const float p0 = ((V.A[0] * x + V.A[1] * y) + V.A[2] * z) + V.b[0];
    const float p1 = ((V.A[3] * x + V.A[4] * y) + V.A[5] * z) + V.b[1];
    const float u = V.fx * (p0 / zc) + V.cx;
    const float q = V.fy * (p1 / zc) + V.cy;
    const float c = floorf(u + 0.5f), r = floorf(q + 0.5f);
    if (!(c >= 0.0f && c <= I.cmax && r >= 0.0f && r <= I.rmax)) return false;
    px = ((uint32_t)v * (uint32_t)I.h + (uint32_t)(int)r) * (uint32_t)I.w + (uint32_t)(int)c;
    const float d = I.depth[px];
    if (!(fabsf(d) < INFINITY && d > 0.0f)) return false;
    if (I.mask && I.mask[px] == 0) return false;
    s = d - zc;
    return true;
}

// ---- host ----------------------------------------------------------------------------------------------------------
// What the sweeps' entry points ask of their volume, images and cameras; 0 or refuse(who, ...).
static inline int check_projective_views(const char *who, int X, int Y, int Z, const double *origin, double res, int n,
                                         int max_views, const double *K, const double *E, int h, int w, float max_weight,
                                         float near)
{
    if (n < 1 || n > max_views) return refuse(who, "n must be 1..MAX_VIEWS views");
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    if (h <= 0 || w <= 0) return refuse(who, "non-positive image size");
    if ((int64_t)n * h * w > 0x7fffffffLL || h > (1 << 24) || w > (1 << 24)) return refuse(who, "images too large");
    if (!(max_weight >= 1.0f && max_weight <= 2048.0f)) return refuse(who, "max_weight must be in 1..2048");
    if (!(near >= 0.0f) || !std::isfinite(near)) return refuse(who, "near must be >= 0 and finite");
    if (!all_finite(origin, 3) || !std::isfinite(res) || !all_finite(K, 9 * n) || !all_finite(E, 12 * n))
        return refuse(who, "non-finite K, E, origin or resolution");
    if (!(res > 0.0)) return refuse(who, "resolution must be > 0");
    for (int v = 0; v < n; ++v) {
        const double *Kv = K + 9 * v;
        if (Kv[1] != 0.0 || Kv[3] != 0.0 || Kv[6] != 0.0 || Kv[7] != 0.0 || Kv[8] != 1.0)
            return refuse(who, "K must be a pinhole matrix [fx 0 cx; 0 fy cy; 0 0 1]");
    }
    return 0;
}

// the host part of the definition, f64, every operation rounded on its own
static inline void make_proj_view(const double *Kv, const double *Ev, const double *origin, double res, ProjView &V)
{
    double gm[3];
    for (int m = 0; m < 3; ++m) gm[m] = (origin[m] + 0.5 * res) - Ev[4 * m + 3];
    for (int a = 0; a < 3; ++a) {
        for (int m = 0; m < 3; ++m) V.A[3 * a + m] = (float)(Ev[4 * m + a] * res);
        V.b[a] = (float)((Ev[a] * gm[0] + Ev[4 + a] * gm[1]) + Ev[8 + a] * gm[2]);
    }
    V.fx = (float)Kv[0]; V.fy = (float)Kv[4]; V.cx = (float)Kv[2]; V.cy = (float)Kv[5];
}

static inline void make_proj_views(const double *K, const double *E, const double *origin, double res, int n, ProjView *V)
{
    for (int v = 0; v < n; ++v) make_proj_view(K + 9 * v, E + 12 * v, origin, res, V[v]);
}

static inline void fill_proj_images(ProjImages &I, const float *depth, const uint8_t *mask, int h, int w, float near)
{
    I.depth = depth; I.mask = mask; I.h = h; I.w = w; I.near = near;
    I.cmax = (float)(w - 1); I.rmax = (float)(h - 1);
}

}  // namespace ojf
