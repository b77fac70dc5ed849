// FRAMES: the live depth frame made ready for tracking and fusion (KinectFusion's first stage) - validity, rejection of the
// mixed pixels at depth edges, a bilateral filter, the camera-space vertex / normal map and an incidence-angle test, for n
// frames [n,h,w] in one launch.  Own definition (the reference only erodes its depth maps, deps/mesh-fusion/2_fusion.py);
// tests/frames_ref.py restates it in numpy and the GPU tests pin the kernel to it bit for bit.
//
// Normative definition.  All device arithmetic is fp32 with every product, sum, division and square root rounded on its
// own (the build's -ffp-contract=off and correctly rounded division / sqrt); the device evaluates no transcendental.  (r, c)
// is a pixel of one frame, d its raw depth; a pixel outside the image is never a neighbour.  "a(p)" is the value a of pixel p.
//
//   1. Validity.  v0 = isfinite(d) and near <= d and d <= far and (no mask or mask != 0).  From here on d = 0 where not v0.
//   2. Edge rejection (off when edge_abs == 0 and edge_rel == 0: v1 = v0).  For a v0 pixel t = edge_abs + edge_rel * d; it
//      loses validity if any of its 8 neighbours p with v0(p) has |d(p) - d| > t.  v1 is what remains; the test reads v0 of
//      the neighbours, never v1: one pass, no cascade.
//   3. Bilateral filter, radius R in 0..4, for a v1 pixel (f = 0 elsewhere).  R == 0: f = d.  Else rho = range0 +
//      range2 * (d * d), q = 1 / rho, num = den = 0, and over the window dr = -R..R (outer), dc = -R..R (inner), k counting
//      the taps from 0, the centre included like any other tap: for a neighbour p = (r + dr, c + dc) with v1(p):
//          diff = d(p) - d;  t = diff * q;  u = 1 - t * t;  if |t| < 1:  wgt = S[k] * (u * u);  num = num + wgt * diff;
//          den = den + wgt.
//      f = d + num / den.  S is the host's f32 table of (2R+1)^2 spatial weights (exp(-(dr^2 + dc^2) / (2 sigma^2)) in f64,
//      rounded once); S[centre] == 1, so den >= 1.
//   4. Vertex and normal map (only when normals are asked for or cos_min != 0), for a v1 pixel, with the frame's
//      (ifx, ify, cx, cy) = (f32(1/fx), f32(1/fy), f32(cx), f32(cy)) from the host:
//          V(p) = (((float(c) - cx) * ifx) * f(p),  ((float(r) - cy) * ify) * f(p),  f(p)).
//      Along the column axis, with p+ = (r, c + 1) and p- = (r, c - 1):  a = V(p+) - V(p-) if v1(p+) and v1(p-);
//      V(p+) - V(p) if only v1(p+);  V(p) - V(p-) if only v1(p-);  otherwise the pixel has no normal.  b likewise along the
//      row axis (r + 1, r - 1).  m = a x b:  m0 = a1 * b2 - a2 * b1,  m1 = a2 * b0 - a0 * b2,  m2 = a0 * b1 - a1 * b0;
//      len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);  no normal unless len > 0 and len finite;  nrm_i = m_i / len;
//      dot = (nrm0 * V0 + nrm1 * V1) + nrm2 * V2;  if dot > 0: nrm = -nrm, dot = -dot.  (A camera-space unit normal that
//      faces the camera.)
//   5. Incidence test (off when cos_min == 0).  cos = (-dot) / sqrt((V0 * V0 + V1 * V1) + V2 * V2);  the pixel stays valid
//      only if it has a normal and cos >= cos_min (a NaN fails).
//   6. Outputs, every element written exactly once:  valid = v1 and the incidence test;  depth_out = f where valid, else 0;
//      valid_out = valid as 0 / 1;  normals_out = nrm where valid and the pixel has a normal, else (0, 0, 0).
//
// Shape.  One launch per call (per kFramesPerLaunch frames).  A workgroup of 256 lanes takes a kTileW x kTileH = 32 x 8 pixel
// tile of one frame (frames on the grid's z axis), one output pixel per lane, and keeps everything between the raw frame and
// the outputs in LDS: it stages the raw tile with the halo the switched-on stages need - R for the filter, + 1 for the edge
// test, + 1 for the normals' differences, R + 2 at the most - then v1 on the halo R + 1 (or R), f on the halo 1 (or 0), and
// from those the normals and the final validity, with a workgroup barrier between the steps.  A stage that is off shrinks the
// halo and is skipped by one uniform branch.  The four LDS arrays are indexed in the frame of the largest halo (20 x 44
// entries, 8.6 KiB per workgroup: LDS never limits occupancy, and a 320 x 240 frame is 300 workgroups - one wave of
// workgroups on the chip's 256 CUs; a larger tile would leave CUs idle at the frame sizes in use, a smaller one stages more
// halo than tile).  With one workgroup per CU a wave waits for nothing but its own LDS reads, so the filter window and the
// edge test are unrolled per radius and free of branches (measured: 15.0 -> 9.0 us per 320 x 240 frame with every stage on at
// radius 2, 31.3 -> 14.4 us at radius 4).  No global intermediate, no atomics, no workspace, no block waits for another: the bits are the same on
// every run and for every split of the n frames into calls.  An output never aliases an input: a tile reads its neighbours'
// pixels, so in-place operation is refused.
#include <cmath>

#include "ojf_common.h"

namespace ojf {

constexpr int kTileW = 32, kTileH = 8;
constexpr int kFramesBlock = kTileW * kTileH;
constexpr int kMaxRadius = 4;
constexpr int kMaxHalo = kMaxRadius + 2;
constexpr int kPitch = kTileW + 2 * kMaxHalo;  // 44
constexpr int kRows = kTileH + 2 * kMaxHalo;   // 20
constexpr int kFramesPerLaunch = 64;           // the by-value intrinsics stay well inside the kernel-argument segment

struct FrameK { float ifx, ify, cx, cy; };

struct FramesLaunch {
    const float *depth;   // of the launch's first frame
    const uint8_t *mask;  // or NULL
    float *depth_out;
    uint8_t *valid_out;   // or NULL
    float *normals_out;   // or NULL
    int h, w, radius;
    int edge, need_normals;
    float range0, range2, edge_abs, edge_rel, near, far, cos_min;
    float S[(2 * kMaxRadius + 1) * (2 * kMaxRadius + 1)];
    FrameK K[kFramesPerLaunch];
};

// LDS index of the pixel at offset (y, x) from the tile's first pixel, -kMaxHalo <= y, x
__device__ __forceinline__ int lds_at(int y, int x) { return (y + kMaxHalo) * kPitch + (x + kMaxHalo); }

// Step 3 for the v1 pixel at LDS index `at`, R > 0.  The window is unrolled and free of branches - a tap that does not count
// is computed and not selected - so that its (2R+1)^2 pairs of LDS reads are in flight together instead of one round trip
// per tap; every tap lies inside the staged halo, where d and v1 are defined (d = 0 where not v0).
template <int R>
__device__ __forceinline__ float bilateral(const float *s_d, const uint8_t *v1, int at, const FramesLaunch &L)
{
    constexpr int side = 2 * R + 1;
    const float d = s_d[at];
    const float rho = L.range0 + L.range2 * (d * d);
    const float q = 1.0f / rho;
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const int p = at + dy * kPitch + dx;
            const float diff = s_d[p] - d;
            const float t = diff * q;
            const float u = 1.0f - t * t;
            const bool take = (v1[p] != 0) & (fabsf(t) < 1.0f);
            const float wgt = L.S[(dy + R) * side + (dx + R)] * (u * u);
            num = take ? num + wgt * diff : num;
            den = take ? den + wgt : den;
        }
    return d + num / den;
}

__global__ __launch_bounds__(kFramesBlock) void frames_kernel(FramesLaunch L)
{
    __shared__ float s_d[kRows * kPitch];    // step 1's d
    __shared__ float s_f[kRows * kPitch];    // step 3's f
    __shared__ uint8_t s_v0[kRows * kPitch];
    __shared__ uint8_t s_v1[kRows * kPitch];

    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * kTileH, c0 = blockIdx.x * kTileW;
    const int h = L.h, w = L.w, R = L.radius;
    const size_t frame = (size_t)blockIdx.z * (size_t)h * (size_t)w;
    const int hf = L.need_normals ? 1 : 0;  // halo of f
    const int h1 = R + hf;                  // halo of v1
    const int h0 = h1 + (L.edge ? 1 : 0);   // halo of the raw tile

    // 1. the raw tile and v0
    {
        const int pw = kTileW + 2 * h0, cnt = (kTileH + 2 * h0) * pw;
        for (int i = tid; i < cnt; i += kFramesBlock) {
            const int y = i / pw - h0, x = i % pw - h0;
            const int r = r0 + y, c = c0 + x;
            float d = 0.0f;
            bool v = false;
            if (r >= 0 && r < h && c >= 0 && c < w) {
                const size_t px = frame + (size_t)r * w + c;
                d = L.depth[px];
                v = fabsf(d) < INFINITY && L.near <= d && d <= L.far && (!L.mask || L.mask[px] != 0);
                if (!v) d = 0.0f;
            }
            s_d[lds_at(y, x)] = d;
            s_v0[lds_at(y, x)] = v;
        }
    }
    __syncthreads();

    // 2. edge rejection: v1 on the halo h1
    const uint8_t *v1 = s_v0;
    if (L.edge) {
        const int pw = kTileW + 2 * h1, cnt = (kTileH + 2 * h1) * pw;
        for (int i = tid; i < cnt; i += kFramesBlock) {
            const int y = i / pw - h1, x = i % pw - h1;
            const int at = lds_at(y, x);
            bool v = s_v0[at];
            if (v) {
                const float d = s_d[at];
                const float t = L.edge_abs + L.edge_rel * d;
                bool drop = false;  // (no branch per neighbour: the nine pairs of LDS reads go out together)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int p = at + dy * kPitch + dx;
                        drop |= (s_v0[p] != 0) & (fabsf(s_d[p] - d) > t);
                    }
                v = !drop;
            }
            s_v1[at] = v;
        }
        v1 = s_v1;
        __syncthreads();
    }

    // 3. bilateral filter: f on the halo hf
    {
        const int pw = kTileW + 2 * hf, cnt = (kTileH + 2 * hf) * pw;
        for (int i = tid; i < cnt; i += kFramesBlock) {
            const int y = i / pw - hf, x = i % pw - hf;
            const int at = lds_at(y, x);
            float f = 0.0f;
            if (v1[at]) {
                const float d = s_d[at];
                f = d;
                switch (R) {
                case 1: f = bilateral<1>(s_d, v1, at, L); break;
                case 2: f = bilateral<2>(s_d, v1, at, L); break;
                case 3: f = bilateral<3>(s_d, v1, at, L); break;
                case 4: f = bilateral<4>(s_d, v1, at, L); break;
                default: break;
                }
            }
            s_f[at] = f;
        }
    }
    __syncthreads();

    // 4.-6. one output pixel per lane
    const int y = tid / kTileW, x = tid % kTileW;
    const int r = r0 + y, c = c0 + x;
    if (r >= h || c >= w) return;
    const int at = lds_at(y, x);
    bool valid = v1[at];
    const float f = s_f[at];
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if (L.need_normals) {
        bool has = false;
        float dot = 0.0f, V[3] = {0.0f, 0.0f, 0.0f};
        if (valid) {
            const FrameK &K = L.K[blockIdx.z];
            // V of the pixel at offset (oy, ox) from this one
            auto vertex = [&](int oy, int ox, float out[3]) {
                const float fp = s_f[at + oy * kPitch + ox];
                out[0] = (((float)(c + ox) - K.cx) * K.ifx) * fp;
                out[1] = (((float)(r + oy) - K.cy) * K.ify) * fp;
                out[2] = fp;
            };
            // the difference along one axis: false if neither neighbour has v1
            auto difference = [&](int oy, int ox, float out[3]) {
                const bool vp = v1[at + oy * kPitch + ox], vm = v1[at - oy * kPitch - ox];
                if (!vp && !vm) return false;
                float P[3], M[3];
                if (vp) vertex(oy, ox, P); else vertex(0, 0, P);
                if (vm) vertex(-oy, -ox, M); else vertex(0, 0, M);
#pragma unroll
                for (int k = 0; k < 3; ++k) out[k] = P[k] - M[k];
                return true;
            };
            vertex(0, 0, V);
            float a[3], b[3];
            if (difference(0, 1, a) && difference(1, 0, b)) {
                const float m[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
                const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
                if (len > 0.0f && len < INFINITY) {
                    has = true;
#pragma unroll
                    for (int k = 0; k < 3; ++k) nrm[k] = m[k] / len;
                    dot = (nrm[0] * V[0] + nrm[1] * V[1]) + nrm[2] * V[2];
                    if (dot > 0.0f) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) nrm[k] = -nrm[k];
                        dot = -dot;
                    }
                }
            }
        }
        if (L.cos_min != 0.0f) {
            const float cs = (-dot) / sqrtf((V[0] * V[0] + V[1] * V[1]) + V[2] * V[2]);
            valid = valid && has && cs >= L.cos_min;
        }
        if (!(valid && has)) nrm[0] = nrm[1] = nrm[2] = 0.0f;
    }
    const size_t px = frame + (size_t)r * w + c;
    L.depth_out[px] = valid ? f : 0.0f;
    if (L.valid_out) L.valid_out[px] = valid;
    if (L.normals_out) {
        float *o = L.normals_out + 3 * px;
        o[0] = nrm[0]; o[1] = nrm[1]; o[2] = nrm[2];
    }
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

}  // namespace ojf

OJF_API int ojf_depth_prepare(const float *depth, const uint8_t *mask, int n, int h, int w, const float *K, int radius,
                              const float *spatial, float range0, float range2, float edge_abs, float edge_rel, float near,
                              float far, float cos_min, float *depth_out, uint8_t *valid_out, float *normals_out,
                              ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_depth_prepare";
    if (!depth || !depth_out) return refuse(who, "null pointer argument");
    if (n < 1 || h < 1 || w < 1) return refuse(who, "n, h and w must be >= 1");
    if ((int64_t)n * h * w > 0x7fffffffLL || (h + kTileH - 1) / kTileH > 65535) return refuse(who, "images too large");
    if (radius < 0 || radius > kMaxRadius) return refuse(who, "radius must be 0..4");
    if (!(range0 > 0.0f) || !std::isfinite(range0) || !(range2 >= 0.0f) || !std::isfinite(range2))
        return refuse(who, "range0 > 0 and range2 >= 0, both finite, expected");
    if (!(edge_abs >= 0.0f) || !std::isfinite(edge_abs) || !(edge_rel >= 0.0f) || !std::isfinite(edge_rel))
        return refuse(who, "edge_abs >= 0 and edge_rel >= 0, both finite, expected");
    if (!(near >= 0.0f) || !std::isfinite(near) || !(far >= near)) return refuse(who, "0 <= near <= far and a finite near expected");
    if (!(cos_min >= 0.0f && cos_min <= 1.0f)) return refuse(who, "cos_min must be in 0..1");
    const bool need_normals = normals_out || cos_min != 0.0f;
    if (need_normals && !K) return refuse(who, "K_host is needed for normals and for cos_min != 0");
    const int taps = (2 * radius + 1) * (2 * radius + 1);
    if (radius > 0) {
        if (!spatial) return refuse(who, "spatial_host is needed for radius > 0");
        for (int i = 0; i < taps; ++i)
            if (!(spatial[i] >= 0.0f && spatial[i] <= 1.0f)) return refuse(who, "spatial weights must be in 0..1");
        if (spatial[taps / 2] != 1.0f) return refuse(who, "the centre's spatial weight must be 1");
    }
    if (K)
        for (int i = 0; i < 4 * n; ++i)
            if (!std::isfinite(K[i])) return refuse(who, "non-finite K_host");
    if (((uintptr_t)depth & 3) || ((uintptr_t)depth_out & 3) || ((uintptr_t)normals_out & 3))
        return refuse(who, "depth_dev, depth_out_dev and normals_out_dev must be 4-byte aligned");
    const size_t px = (size_t)n * h * w;
    const void *in[2] = {depth, mask};
    const size_t in_bytes[2] = {4 * px, px};
    const void *out[3] = {depth_out, valid_out, normals_out};
    const size_t out_bytes[3] = {4 * px, px, 12 * px};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 2; ++j)
            if (overlap(out[i], out_bytes[i], in[j], in_bytes[j]))
                return refuse(who, "an output overlaps an input (a tile reads its neighbours' pixels: no in-place operation)");
        for (int j = i + 1; j < 3; ++j)
            if (overlap(out[i], out_bytes[i], out[j], out_bytes[j])) return refuse(who, "two outputs overlap");
    }

    FramesLaunch L;
    L.h = h; L.w = w; L.radius = radius;
    L.edge = edge_abs != 0.0f || edge_rel != 0.0f;
    L.need_normals = need_normals;
    L.range0 = range0; L.range2 = range2; L.edge_abs = edge_abs; L.edge_rel = edge_rel;
    L.near = near; L.far = far; L.cos_min = cos_min;
    for (int i = 0; i < (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1); ++i) L.S[i] = radius > 0 && i < taps ? spatial[i] : 0.0f;
    const dim3 tiles((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH);
    for (int v0 = 0; v0 < n; v0 += kFramesPerLaunch) {
        const int nv = n - v0 < kFramesPerLaunch ? n - v0 : kFramesPerLaunch;
        const size_t first = (size_t)v0 * h * w;
        L.depth = depth + first;
        L.mask = mask ? mask + first : nullptr;
        L.depth_out = depth_out + first;
        L.valid_out = valid_out ? valid_out + first : nullptr;
        L.normals_out = normals_out ? normals_out + 3 * first : nullptr;
        for (int j = 0; j < kFramesPerLaunch; ++j) {
            const float *k = K && j < nv ? K + 4 * (size_t)(v0 + j) : nullptr;
            L.K[j] = k ? FrameK{k[0], k[1], k[2], k[3]} : FrameK{0.0f, 0.0f, 0.0f, 0.0f};
        }
        hipLaunchKernelGGL(frames_kernel, dim3(tiles.x, tiles.y, nv), dim3(kFramesBlock), 0, as_stream(stream), L);
        OJF_HIP(hipGetLastError());
    }
    return 0;
}
