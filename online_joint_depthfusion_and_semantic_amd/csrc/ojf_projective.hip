// PROJECTIVE: classical voxel-projective TSDF fusion (Curless-Levoy / KinectFusion style) of n depth views into the fp16
// volumes, without a network.  Own definition (the reference fuses through FusionNet only); tests/projective_ref.py
// restates it in numpy and the GPU tests pin the kernel to it bit for bit.
//
// Normative definition.  All device arithmetic is fp32 with every product, sum and division rounded on its own (the
// build's -ffp-contract=off and correctly rounded division); "(a + b) + c" order is as written; fp16 conversions round to
// nearest even.  Volume frame: voxel (i,j,k) has its centre at origin + (i+0.5, j+0.5, k+0.5)·res (the frame of extract /
// integrate / render).
//   Host, per view, in f64, every operation rounded separately, in this order (E: camera-to-world, 3x4 row-major, assumed
//   rigid - R^T serves as the inverse, unchecked):
//     R[m][a] = E[4m+a], t_m = E[4m+3];   g_m = (origin_m + 0.5·res) - t_m
//     A[a][m] = fp32(R[m][a]·res);        b_a = fp32((R[0][a]·g_0 + R[1][a]·g_1) + R[2][a]·g_2)
//     fx = fp32(K[0]), fy = fp32(K[4]), cx = fp32(K[2]), cy = fp32(K[5]); a K whose other entries are not 0,0,0,0,1 is
//     refused.
//   Per voxel (i,j,k), for views v = 0..n-1 in that order (x, y, z: the indices as floats; "skip": this view leaves the
//   voxel alone):
//     1. p_a = ((A[a][0]·x + A[a][1]·y) + A[a][2]·z) + b_a;  zc = p_2;  skip unless zc > near.
//     2. u = fx·(p_0 / zc) + cx,  q = fy·(p_1 / zc) + cy;  c = floor(u + 0.5), r = floor(q + 0.5);  skip unless
//        0 <= c <= w-1 and 0 <= r <= h-1 (float comparisons, before any conversion to int: a NaN or inf fails them).
//     3. d = depth[v][r][c];  skip unless d is finite, d > 0 and the mask is NULL or non-zero at that pixel.
//     4. s = d - zc (the projective distance along the optical axis);  skip if s < -trunc;  if s > trunc, skip when
//        carve == 0;  band = (s <= trunc).
//     5. o = min(s, trunc);  w0 = float(W), t0 = float(T):  w1 = w0 + 1,  t1 = (w0·t0 + o) / w1;
//        T = half(t1),  W = half(min(w1, max_weight)).
//     6. only with label images and id / score volumes, and only if band:  sc = half(label_scores ? label_scores[v][r][c]
//        : 1.0f);  if float(sc) > float(S): ids = labels[v][r][c], S = sc (the reference integrator's "new score beats
//        old score" rule, modules/integrator.py:110-116).
//   trunc > 0 finite; 1 <= max_weight <= 2048 (fp16 is exact on those integers); near >= 0; carve in {0, 1}: 0 writes the
//   truncation band only (like the learned integrator: Database.filter / evaluate masks stay comparable), 1 also pulls the
//   free space in front of the surface to +trunc (what a live stream needs to erase stale geometry).
//
// Shape: every voxel is owned by one lane for the whole call; a lane owns 8 consecutive voxels of the flattened volume
// (16 B of TSDF, 16 B of weights, 8 B of ids, 16 B of scores; lanes run along the contiguous z axis) and walks the n views
// in order with the voxels' fp16 bits in registers.  The 16-byte loads are issued lazily, once some voxel of the group
// has a view that reaches step 5 (ids / scores: step 6), and a group is stored only if it was loaded: the sweep neither
// reads nor writes the volume outside what the views touch.  Values are rounded to fp16 after every view, so n views in
// one call give the bits of n calls of one view.  No atomics, no LDS, no workspace: every run repeats its bits.
// The last group of a volume whose size is no multiple of 8, and every group of a volume whose pointers are not aligned
// for the wide accesses, go element by element.
// The host constants and steps 1-3 are in ojf_projview.h, shared with the colour sweep (ojf_color.hip).
#include "ojf_projview.h"

namespace ojf {

constexpr int kProjGroup = 8;
constexpr int kProjBlock = 256;

struct ProjArgs {
    uint16_t *tsdf, *wgt;
    uint8_t *ids;      // NULL: geometry only
    uint16_t *scores;
    ProjImages im;
    const uint8_t *labels;
    const float *lscores;
    uint32_t total, groups;
    int Y, Z, n, carve, vec;
    float trunc, max_weight;
};

struct ProjLaunch {
    ProjArgs a;
    ProjView v[OJF_PROJECTIVE_MAX_VIEWS];
};

__device__ __forceinline__ void load16x8(const uint16_t *p, bool vec, int cnt, uint32_t q[4])
{
    if (vec) {
        load8(p, 0, q);
    } else {
#pragma unroll
        for (int e = 0; e < kProjGroup; ++e)
            if (e < cnt) set16(q, e, p[e]);
    }
}

__device__ __forceinline__ void store16x8(uint16_t *p, bool vec, int cnt, const uint32_t q[4])
{
    if (vec) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int e = 0; e < kProjGroup; ++e)
            if (e < cnt) p[e] = (uint16_t)get16(q, e);
    }
}

__global__ __launch_bounds__(kProjBlock) void projective_kernel(ProjLaunch L)
{
    const ProjArgs &P = L.a;
    const uint32_t g = blockIdx.x * kProjBlock + threadIdx.x;
    if (g >= P.groups) return;
    const uint32_t first = g * kProjGroup;
    const int cnt = P.total - first < (uint32_t)kProjGroup ? (int)(P.total - first) : kProjGroup;
    const bool vec = P.vec && cnt == kProjGroup;
    const bool sem = P.ids != nullptr;

    float xs[kProjGroup], ys[kProjGroup], zs[kProjGroup];
    voxel_indices<kProjGroup>(first, P.Y, P.Z, xs, ys, zs);

    uint32_t tq[4] = {0, 0, 0, 0}, wq[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0}, iq[2] = {0, 0};
    bool loaded = false, sloaded = false, sdirty = false;

    for (int v = 0; v < P.n; ++v) {
        const ProjView &V = L.v[v];
        float o[kProjGroup];
        uint32_t pix[kProjGroup];
        uint32_t hit = 0, band = 0;
#pragma unroll
        for (int e = 0; e < kProjGroup; ++e) {
            o[e] = 0.0f;
            pix[e] = 0;
            if (e >= cnt) continue;
            uint32_t px;
            float s;
            if (!project_depth(V, P.im, v, xs[e], ys[e], zs[e], px, s)) continue;
            if (s < -P.trunc) continue;
            const bool in_band = s <= P.trunc;
            if (!in_band && !P.carve) continue;
            o[e] = fminf(s, P.trunc);
            pix[e] = px;
            hit |= 1u << e;
            band |= (in_band ? 1u : 0u) << e;
        }
        if (!hit) continue;
        if (!loaded) {
            load16x8(P.tsdf + first, vec, cnt, tq);
            load16x8(P.wgt + first, vec, cnt, wq);
            loaded = true;
        }
#pragma unroll
        for (int e = 0; e < kProjGroup; ++e) {
            if (!((hit >> e) & 1u)) continue;
            const float t0 = h2f((uint16_t)get16(tq, e)), w0 = h2f((uint16_t)get16(wq, e));
            const float w1 = w0 + 1.0f;
            const float t1 = (w0 * t0 + o[e]) / w1;
            set16(tq, e, f2h(t1));
            set16(wq, e, f2h(fminf(w1, P.max_weight)));
        }
        if (sem && band) {
            if (!sloaded) {
                load16x8(P.scores + first, vec, cnt, sq);
                if (vec) {
                    const uint2 r = *reinterpret_cast<const uint2 *>(P.ids + first);
                    iq[0] = r.x; iq[1] = r.y;
                } else {
#pragma unroll
                    for (int e = 0; e < kProjGroup; ++e)
                        if (e < cnt) set8(iq, e, P.ids[first + e]);
                }
                sloaded = true;
            }
#pragma unroll
            for (int e = 0; e < kProjGroup; ++e) {
                if (!((band >> e) & 1u)) continue;
                const uint16_t sc = P.lscores ? f2h(P.lscores[pix[e]]) : (uint16_t)0x3c00;
                if (h2f(sc) > h2f((uint16_t)get16(sq, e))) {
                    set8(iq, e, P.labels[pix[e]]);
                    set16(sq, e, sc);
                    sdirty = true;
                }
            }
        }
    }

    if (loaded) {
        store16x8(P.tsdf + first, vec, cnt, tq);
        store16x8(P.wgt + first, vec, cnt, wq);
    }
    if (sdirty) {
        store16x8(P.scores + first, vec, cnt, sq);
        if (vec) {
            *reinterpret_cast<uint2 *>(P.ids + first) = make_uint2(iq[0], iq[1]);
        } else {
#pragma unroll
            for (int e = 0; e < kProjGroup; ++e)
                if (e < cnt) P.ids[first + e] = (uint8_t)get8(iq, e);
        }
    }
}

}  // namespace ojf

OJF_API int ojf_fuse_projective(uint16_t *tsdf, uint16_t *wgt, uint8_t *ids, uint16_t *scores, int X, int Y, int Z,
                                const double *origin, double res, int n, const double *K, const double *E,
                                const float *depth, const uint8_t *mask, const uint8_t *labels, const float *lscores,
                                int h, int w, float trunc, float max_weight, float near, int carve, ojf_stream_t stream)
{
    using namespace ojf;
    if (!tsdf || !wgt || !origin || !K || !E || !depth) return fail("ojf_fuse_projective: null pointer argument");
    if ((ids != nullptr) != (scores != nullptr) || (ids != nullptr) != (labels != nullptr))
        return fail("ojf_fuse_projective: ids_dev, scores_dev and labels_dev are all given or all null");
    if (lscores && !labels) return fail("ojf_fuse_projective: label_scores_dev needs labels_dev (null otherwise)");
    if (!(trunc > 0.0f) || !std::isfinite(trunc)) return fail("ojf_fuse_projective: trunc must be > 0 and finite");
    if (carve != 0 && carve != 1) return fail("ojf_fuse_projective: carve must be 0 or 1");
    if (int rc = check_projective_views("ojf_fuse_projective", X, Y, Z, origin, res, n, OJF_PROJECTIVE_MAX_VIEWS, K, E, h, w, max_weight, near))
        return rc;
    ProjLaunch L;
    ProjArgs &A = L.a;
    A.tsdf = tsdf; A.wgt = wgt; A.ids = ids; A.scores = scores;
    fill_proj_images(A.im, depth, mask, h, w, near);
    A.labels = labels; A.lscores = lscores;
    A.total = (uint32_t)((int64_t)X * Y * Z);
    A.groups = (A.total + kProjGroup - 1) / kProjGroup;
    A.Y = Y; A.Z = Z; A.n = n; A.carve = carve;
    // the wide accesses need 16-byte aligned fp16 volumes and an 8-byte aligned id volume; anything else goes element by element
    A.vec = (((uintptr_t)tsdf | (uintptr_t)wgt | (uintptr_t)scores) & 15) == 0 && ((uintptr_t)ids & 7) == 0;
    A.trunc = trunc; A.max_weight = max_weight;
    make_proj_views(K, E, origin, res, n, L.v);
    const uint32_t blocks = (A.groups + kProjBlock - 1) / kProjBlock;
    hipLaunchKernelGGL(projective_kernel, dim3(blocks), dim3(kProjBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    return 0;
}
