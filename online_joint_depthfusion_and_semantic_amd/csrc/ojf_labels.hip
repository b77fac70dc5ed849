// LABELS: a per-voxel class distribution beside the fused geometry (SemanticFusion / Kimera-Semantics style) - every voxel
// keeps the running mean of the class probabilities the views bring, and its label is the arg max of that mean, in place
// of the reference's one-slot rule (one (id, score) pair per voxel, replaced when a higher score arrives: one confident
// wrong pixel owns a voxel for good).  Fusion is the voxel-projective sweep of ojf_projective.hip / ojf_color.hip; the
// decision is one pass that writes into the id / score volumes everything downstream already reads.  Own definition (the
// reference has no counterpart); tests/label_ref.py restates it in numpy and the GPU tests pin the kernels to it bit for
// bit.
//
// The volume: fp16 [X,Y,Z,S], voxel-major, 16-byte aligned, S = 8·ceil((C+1)/8) for C classes (2 <= C <= 256): a voxel's
// record is S/8 chunks of 16 bytes.  Channels 0..C-1: P_k, the running mean of the probability of class k; channel C: the
// weight W; W == 0: nothing fused; all zeros at reset.  Channels C+1..S-1 are padding that no kernel reads or writes.
// The frame is the one of extract / integrate / render / projective: voxel (i,j,k) has its centre at origin + (i+0.5,
// j+0.5, k+0.5)·res.
//
// Normative definition.  All device arithmetic is fp32 with every product, sum and division rounded on its own (the
// build's -ffp-contract=off and correctly rounded division); fp16 conversions round to nearest even; min is IEEE minNum.
//
// ojf_fuse_label_probs, per voxel (i,j,k), for views v = 0..n-1 in that order ("skip": this view leaves the voxel alone):
//     1. steps 1-3 of ojf_fuse_projective exactly (ojf_projview.h: the same host f64 constants, the same projection,
//        nearest pixel floor(u + 0.5), float bounds checks, depth and mask tests) give the pixel px and its depth d, and zc.
//     2. s = d - zc;  skip unless -band <= s <= band (labels are written near the observed surface only; no carving).
//     3. the observation p_k, k = 0..C-1, in one of two forms:
//          probabilities  x = probs[px·prob_stride + k];  p_k = (x >= 0 && x <= 1) ? x : 0  (a NaN counts as 0);
//          labels         l = labels[px];  skip if l >= C;  p_k = (k == l) ? 1 : 0.
//     4. w0 = float(W), w1 = w0 + 1;  for k = 0..C-1:  P_k = half((w0·float(P_k) + p_k) / w1).
//     5. W = half(min(w1, max_weight)).
//   band > 0 finite; 1 <= max_weight <= 2048; near >= 0.  The TSDF and weight volumes are never read.
//
// ojf_label_decide, per voxel: skip unless float(W) > 0 (a W of 0, -0, a negative value or a NaN leaves ids / scores as
//     they are: labels written outside the band by the learned integrator survive).  Else best = float(P_0), id = 0; for
//     k = 1..C-1 in order: if float(P_k) > best: best = float(P_k), id = k (the smallest k of the maximum);
//     ids[voxel] = id, scores[voxel] = the fp16 bits of P_id.
//
// Shape.  Fusion: one lane owns one voxel for the whole call (lanes run along the contiguous z axis) and walks the n views
// in order.  The projection of every (voxel, view) is the bulk of the sweep; only the voxels inside the band of a view
// (1-2 % of a room) touch their record, and they do it per view (record_fuse, ojf_records.h, shared with the depth
// histograms of ojf_tvl1.hip): a read-modify-write of the record straight in memory -
// C/8 whole chunks as 16-byte accesses, then the C mod 8 classes of the last chunk and W as 2-byte accesses, which is
// what keeps the padding unread.  Nothing of the record is held across views (C = 256 is 132 dwords; values are rounded
// to fp16 after every view anyway, so n views in one call give the bits of n calls of one view), the same lane reads what
// it stored in program order, and the kernel needs 4 dwords of record at a time whatever C is.  No atomics, no LDS, no
// workspace, one launch.  The decision: one lane per voxel, W first, the record only where W > 0.
#include "ojf_projview.h"
#include "ojf_records.h"

namespace ojf {

constexpr int kLabelBlock = 256;

struct LabelArgs {
    uint16_t *vol;
    ProjImages im;
    const float *probs;     // f32 [n,h,w] rows of prob_stride floats, or null
    const uint8_t *labels;  // u8 [n,h,w], or null
    uint32_t total;
    int Y, Z, n, C, S, prob_stride;
    float band, max_weight;
};

struct LabelLaunch {
    LabelArgs a;
    ProjView v[OJF_LABEL_MAX_VIEWS];
};

// step 3's clamp of a probability
__device__ __forceinline__ float label_prob(float x) { return (x >= 0.0f && x <= 1.0f) ? x : 0.0f; }

template <bool PROBS>
__global__ __launch_bounds__(kLabelBlock) void label_fuse_kernel(LabelLaunch L)
{
    const LabelArgs &P = L.a;
    const uint32_t g = blockIdx.x * kLabelBlock + threadIdx.x;
    if (g >= P.total) return;
    float xs[1], ys[1], zs[1];
    voxel_indices<1>(g, P.Y, P.Z, xs, ys, zs);
    uint16_t *const rec = P.vol + (size_t)g * (size_t)P.S;
    for (int v = 0; v < P.n; ++v) {
        uint32_t px;
        float s;
        if (!project_depth(L.v[v], P.im, v, xs[0], ys[0], zs[0], px, s)) continue;
        if (!(s >= -P.band && s <= P.band)) continue;
        if constexpr (PROBS) {
            const float *const row = P.probs + (size_t)px * (size_t)P.prob_stride;
            record_fuse(rec, P.C, P.max_weight, [&](int k) { return label_prob(row[k]); });
        } else {
            const int label = P.labels[px];
            if (label >= P.C) continue;
            record_fuse(rec, P.C, P.max_weight, [&](int k) { return (k == label) ? 1.0f : 0.0f; });
        }
    }
}

struct DecideArgs {
    const uint16_t *vol;
    uint8_t *ids;
    uint16_t *scores;
    uint32_t total;
    int C, S;
};

__global__ __launch_bounds__(kLabelBlock) void label_decide_kernel(DecideArgs P)
{
    const uint32_t g = blockIdx.x * kLabelBlock + threadIdx.x;
    if (g >= P.total) return;
    const uint16_t *const rec = P.vol + (size_t)g * (size_t)P.S;
    if (!(h2f(rec[P.C]) > 0.0f)) return;  // (a NaN fails)
    const int full = P.C >> 3;
    float best = 0.0f;
    uint32_t bits = 0;
    int id = -1;
    auto take = [&](uint32_t b, int k) {
        const float x = h2f((uint16_t)b);
        if (id < 0 || x > best) { best = x; bits = b; id = k; }
    };
    for (int c = 0; c < full; ++c) {
        const uint4 r = reinterpret_cast<const uint4 *>(rec)[c];
        const uint32_t q[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) take(get16(q, e), 8 * c + e);
    }
    for (int k = 8 * full; k < P.C; ++k) take(rec[k], k);
    P.ids[g] = (uint8_t)id;
    P.scores[g] = (uint16_t)bits;
}

static int check_label_volume(const char *who, const void *vol, int C)
{
    if (C < 2 || C > 256) return refuse(who, "n_classes must be in 2..256");
    if ((uintptr_t)vol & 15) return refuse(who, "probs_vol_dev must be 16-byte aligned");
    return 0;
}

}  // namespace ojf

OJF_API int ojf_fuse_label_probs(uint16_t *vol, int n_classes, int X, int Y, int Z, const double *origin, double res, int n,
                                 const double *K, const double *E, const float *depth, const uint8_t *mask, const float *probs,
                                 int prob_stride, const uint8_t *labels, int h, int w, float band, float max_weight, float near,
                                 ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_fuse_label_probs";
    if (!vol || !origin || !K || !E || !depth) return refuse(who, "null pointer argument");
    if ((probs != nullptr) == (labels != nullptr)) return refuse(who, "exactly one of probs_dev and labels_dev must be given");
    if (int rc = check_label_volume(who, vol, n_classes)) return rc;
    if (probs && prob_stride < n_classes) return refuse(who, "prob_stride must be >= n_classes");
    if (!(band > 0.0f) || !std::isfinite(band)) return refuse(who, "band must be > 0 and finite");
    if (int rc = check_projective_views(who, X, Y, Z, origin, res, n, OJF_LABEL_MAX_VIEWS, K, E, h, w, max_weight, near)) return rc;
    if (probs && ((uintptr_t)probs & 3)) return refuse(who, "probs_dev must be 4-byte aligned");
    LabelLaunch L;
    LabelArgs &A = L.a;
    A.vol = vol;
    fill_proj_images(A.im, depth, mask, h, w, near);
    A.probs = probs; A.labels = labels;
    A.total = (uint32_t)((int64_t)X * Y * Z);
    A.Y = Y; A.Z = Z; A.n = n; A.C = n_classes; A.S = record_size(n_classes); A.prob_stride = prob_stride;
    A.band = band; A.max_weight = max_weight;
    make_proj_views(K, E, origin, res, n, L.v);
    const uint32_t blocks = (A.total + kLabelBlock - 1) / kLabelBlock;
    if (probs) hipLaunchKernelGGL(label_fuse_kernel<true>, dim3(blocks), dim3(kLabelBlock), 0, as_stream(stream), L);
    else hipLaunchKernelGGL(label_fuse_kernel<false>, dim3(blocks), dim3(kLabelBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_label_decide(const uint16_t *vol, int n_classes, int X, int Y, int Z, uint8_t *ids, uint16_t *scores,
                             ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_label_decide";
    if (!vol || !ids || !scores) return refuse(who, "null pointer argument");
    if (int rc = check_label_volume(who, vol, n_classes)) return rc;
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    if ((uintptr_t)scores & 1) return refuse(who, "scores_dev must be 2-byte aligned");
    DecideArgs A;
    A.vol = vol; A.ids = ids; A.scores = scores;
    A.total = (uint32_t)((int64_t)X * Y * Z);
    A.C = n_classes; A.S = record_size(n_classes);
    const uint32_t blocks = (A.total + kLabelBlock - 1) / kLabelBlock;
    hipLaunchKernelGGL(label_decide_kernel, dim3(blocks), dim3(kLabelBlock), 0, as_stream(stream), A);
    OJF_HIP(hipGetLastError());
    return 0;
}
