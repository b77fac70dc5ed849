// RASTER: depth, face, label and colour images of a triangle mesh at n pinhole views - the way from a mesh to frames and,
// through ojf_fuse_projective with carve, to a ground-truth volume.  (The reference makes its ground truth with an OpenGL
// off-screen renderer feeding a CUDA fusion; neither is used here.)  Own definition; tests/raster_ref.py restates it in
// numpy, every pixel against every triangle, and the GPU tests pin the kernels to it bit for bit.
//
// Normative definition.  All device arithmetic is fp32 with every product, sum and division rounded on its own (the
// build's -ffp-contract=off and correctly rounded division).
//
// Inputs: vertices f32 [nv][3] in the world frame, faces i32 [nf][3]; per view a pinhole K and a camera-to-world E in the
// conventions of check_projective_views (ojf_projview.h).  Pixel (r, c) has its centre at integer coordinates, as in
// project_depth.
//   host:    R[m][a] = (float)E[4m+a],  t[m] = (float)E[4m+3],  fx, fy, cx, cy = (float)K[0], K[4], K[2], K[5].
//   camera point of a vertex P:  d = P - t component-wise;  a_k = (R[0][k]·d0 + R[1][k]·d1) + R[2][k]·d2.
//   pixel ray:  rx = ((float)c - cx) / fx,  ry = ((float)r - cy) / fy;  the ray is (rx, ry, 1).
//   triangle with camera points a, b, c in face order:
//       n0 = b×c, n1 = c×a, n2 = a×b  with  u×v = (u1·v2 - u2·v1, u2·v0 - u0·v2, u0·v1 - u1·v0);
//       det = (a0·n0x + a1·n0y) + a2·n0z;
//       e_i = (n_i.x·rx + n_i.y·ry) + n_i.z;   S = (e0 + e1) + e2;   z = det / S.
//   acceptance: all e_i >= 0 or all e_i <= 0 (two-sided, no culling), S != 0, z finite and z > near.
//   visibility: key = (bits(z) << 32) | face index, as a u64; a pixel keeps the minimum key - the nearest hit, ties to the
//       lower face index.  depth f32 [n,h,w]: z of the kept key, 0 where nothing is hit; face i32 [n,h,w]: its face, -1
//       where nothing is hit.
//   skipped faces: an index outside [0, nv), or a vertex with a non-finite world coordinate.  (NaN edge values fail both
//       sign tests on their own.)
// This is homogeneous rasterisation: a triangle that crosses the camera plane needs no clipping.  A shared edge gives
// exactly negated edge values in its two triangles (equal ones under inconsistent winding): the cross product of a
// reversed pair negates bit for bit, so a mesh has no holes along shared edges.
//
// Attributes (ojf_rasterize_attributes), per pixel with f = face[pixel]:  f outside [0, nf), or a face the list above
// skips: label 0, rgba 0.  Else label = face_labels[f];  colour: e_i and S of face f at this pixel by the text above,
// lambda_i = e_i / S;  c_k = (lambda0·C0k + lambda1·C1k) + lambda2·C2k over the u8 colours C0, C1, C2 of the face's vertices in
// face order, k = 0, 1, 2;  byte k = floorf(c_k + 0.5) clamped to 0..255 (a NaN gives 0), alpha 255.
//
// Shape.  The keys are filled with ones.  raster_kernel: one lane per (view, triangle) transforms the three vertices and
// forms n0, n1, n2, det.  z > near >= 0 makes det and S agree in sign, and S has the sign the e_i share: a triangle with
// det == 0 or non-finite is never accepted, and the others only where every e_i·sign(det) >= 0.  When all three camera
// depths are > 0 the lane takes the pixel box of the projected vertices (floor / ceil widened by one pixel, and by more
// for a triangle whose smallest angular height is within rounding of zero - `slack` below -, clamped to the image); a
// triangle wholly behind the camera plane (and well conditioned) is dropped; everything else takes the whole image.
// Three tiers by the size of the box: up to 4 x 4 pixels the lane walks it itself; up to 1024 pixels the whole wave takes
// such triangles one at a time (a loop over __ballot, the triangle broadcast from its lane, 8 x 8 pixel tiles); larger ones -
// screen-filling triangles, and those that cross the camera plane - are appended to a list of (view, face) pairs, and
// raster_large_kernel, a fixed grid whose waves take (pair, band of rows) units in turn, spreads each over 32 waves.  The
// list needs no workspace of its own: it lives in depth_dev / face_dev, which nothing reads before resolve_kernel
// overwrites them (h·w·n - 1 entries; a triangle that finds the list full is swept by its wave, as in the second tier).  A
// candidate key is compared with a plain load first and goes to a 64-bit atomicMin (no return value) only when it is
// smaller; the minimum does not depend on order, so two runs give the same bits whatever the order of the list.
// resolve_kernel turns keys into depth and face.  No host wait.
//
// The box and the rounding of the edge functions.  A pixel the definition accepts lies inside the triangle the rounded
// n_i describe.  Each rounded n_i is off its exact plane by at most a few ulp of its products, which moves the edge's line
// in the image by about eps·F / sin(theta_i) pixels (theta_i: the angle the edge subtends at the camera, F = max(fx, fy)·(1 +
// |r|^2 at the image's farthest corner)), and moves a corner of the triangle by that over the sine of the corner's angle:
// together about eps·F / (the triangle's smallest angular height) = eps·F·max_i(|n_i|·|w_i|) / |det|, w_i the vertex opposite
// edge i.  `est` is four times that with eps = 2^-24; up to est = 0.5 the one-pixel widening covers it, beyond it the box
// grows by ceil(est) pixels (a degenerate triangle ends at the whole image).  This is reasoning about magnitudes, not a
// proof; the GPU tests compare with the box-free reference on meshes with sub-pixel, zero-area and edge-on triangles.
#include "ojf_blocks.h"

namespace ojf {

constexpr int kRasterBlock = 256;
constexpr int kSmallBox = 4;  // boxes up to kSmallBox x kSmallBox pixels are walked by the triangle's own lane
constexpr int kDeferArea = 1024;  // boxes of more pixels go to the list of raster_large_kernel
constexpr int kStrips = 32;  // bands of rows a listed triangle's box is cut into, one per wave
constexpr int kLargeBlocks = 1024;  // grid of raster_large_kernel (the length of the list is not known on the host)

struct RasterView {  // 17 floats, by value in the kernel arguments
    float R[9];      // R[3m+a] = (float)E[4m+a]
    float t[3];
    float fx, fy, cx, cy;
    float slack;  // 4 · 2^-24 · F (see the header)
};

struct RasterMesh {
    const float *vertices;
    const int *faces;
    int nv, nf;
};

struct RasterLaunch {
    RasterMesh m;
    unsigned long long *keys;
    uint32_t *count, *list_view, *list_face;  // the list of large boxes: in the output images, until they are written
    uint32_t cap;
    int h, w;
    float near;
    RasterView v[OJF_RASTER_MAX_VIEWS];
};

struct RasterTri {  // what the pixel test needs of one triangle
    float n0[3], n1[3], n2[3];
    float det;
};

__device__ __forceinline__ void camera_point(const RasterView &V, const float P[3], float a[3])
{
    const float d0 = P[0] - V.t[0], d1 = P[1] - V.t[1], d2 = P[2] - V.t[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = (V.R[k] * d0 + V.R[3 + k] * d1) + V.R[6 + k] * d2;
}

// Face f of the mesh at view V: false for a skipped face; else the camera points and the triangle's constants.
__device__ __forceinline__ bool setup_triangle(const RasterMesh &M, const RasterView &V, int f, float a[3], float b[3], float c[3],
                                               RasterTri &T, int idx[3])
{
    idx[0] = M.faces[3 * (size_t)f]; idx[1] = M.faces[3 * (size_t)f + 1]; idx[2] = M.faces[3 * (size_t)f + 2];
    if ((unsigned)idx[0] >= (unsigned)M.nv || (unsigned)idx[1] >= (unsigned)M.nv || (unsigned)idx[2] >= (unsigned)M.nv) return false;
    float P[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) P[i][k] = M.vertices[3 * (size_t)idx[i] + k];
        if (!finite3(P[i])) return false;
    }
    camera_point(V, P[0], a);
    camera_point(V, P[1], b);
    camera_point(V, P[2], c);
    cross3(b, c, T.n0);
    cross3(c, a, T.n1);
    cross3(a, b, T.n2);
    T.det = (a[0] * T.n0[0] + a[1] * T.n0[1]) + a[2] * T.n0[2];
    return true;
}

__device__ __forceinline__ void edge_values(const RasterView &V, const RasterTri &T, int r, int c, float e[3], float &S)
{
    const float rx = ((float)c - V.cx) / V.fx;
    const float ry = ((float)r - V.cy) / V.fy;
    e[0] = (T.n0[0] * rx + T.n0[1] * ry) + T.n0[2];
    e[1] = (T.n1[0] * rx + T.n1[1] * ry) + T.n1[2];
    e[2] = (T.n2[0] * rx + T.n2[1] * ry) + T.n2[2];
    S = (e[0] + e[1]) + e[2];
}

__device__ __forceinline__ void test_pixel(const RasterView &V, const RasterTri &T, int r, int c, float near, uint32_t face,
                                           unsigned long long *keys /* of the view */, int w)
{
    float e[3], S;
    edge_values(V, T, r, c, e, S);
    const bool pos = e[0] >= 0.0f && e[1] >= 0.0f && e[2] >= 0.0f;
    const bool neg = e[0] <= 0.0f && e[1] <= 0.0f && e[2] <= 0.0f;
    if (!(pos || neg) || S == 0.0f) return;
    const float z = T.det / S;
    if (!(fabsf(z) < INFINITY && z > near)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | face;
    unsigned long long *p = keys + (size_t)r * w + c;
    if (key < *p) atomicMin(p, key);  // (a stale read is only ever too large: one atomic more, the same minimum)
}

struct RasterBox { int r0, r1, c0, c1; };  // pixels, inclusive; r1 < r0: empty

// Face f at view V: its constants and the pixel box outside of which the definition accepts nothing (the header's "shape").
__device__ __forceinline__ RasterBox triangle_box(const RasterMesh &M, const RasterView &V, int f, int h, int w, RasterTri &T)
{
    RasterBox B{0, -1, 0, -1};
    float a[3], b[3], c[3];
    int idx[3];
    if (!(setup_triangle(M, V, f, a, b, c, T, idx) && fabsf(T.det) < INFINITY && T.det != 0.0f)) return B;
    // est of the header: how far rounding can move the triangle's outline, in pixels
    const float na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2],
                nc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    const float m0 = ((T.n0[0] * T.n0[0] + T.n0[1] * T.n0[1]) + T.n0[2] * T.n0[2]) * na;
    const float m1 = ((T.n1[0] * T.n1[0] + T.n1[1] * T.n1[1]) + T.n1[2] * T.n1[2]) * nb;
    const float m2 = ((T.n2[0] * T.n2[0] + T.n2[1] * T.n2[1]) + T.n2[2] * T.n2[2]) * nc;
    const float est = V.slack * (sqrtf(fmaxf(m0, fmaxf(m1, m2))) / fabsf(T.det));
    const bool sound = est <= 0.5f;  // (false for a NaN)
    const float zmin = fminf(a[2], fminf(b[2], c[2])), zmax = fmaxf(a[2], fmaxf(b[2], c[2]));
    if (zmax < 0.0f && sound) return B;  // wholly behind the camera plane: z = det / S < 0 wherever the e_i share a sign
    B = RasterBox{0, h - 1, 0, w - 1};
    if (!(zmin > 0.0f && est < 1.0e6f)) return B;
    const float grow = sound ? 1.0f : 1.0f + ceilf(est);
    const float ua = V.fx * (a[0] / a[2]) + V.cx, ub = V.fx * (b[0] / b[2]) + V.cx, uc = V.fx * (c[0] / c[2]) + V.cx;
    const float va = V.fy * (a[1] / a[2]) + V.cy, vb = V.fy * (b[1] / b[2]) + V.cy, vc = V.fy * (c[1] / c[2]) + V.cy;
    if (!(fabsf(ua) < INFINITY && fabsf(ub) < INFINITY && fabsf(uc) < INFINITY && fabsf(va) < INFINITY && fabsf(vb) < INFINITY &&
          fabsf(vc) < INFINITY))
        return B;
    const float cl = floorf(fminf(ua, fminf(ub, uc))) - grow, ch = ceilf(fmaxf(ua, fmaxf(ub, uc))) + grow;
    const float rl = floorf(fminf(va, fminf(vb, vc))) - grow, rh = ceilf(fmaxf(va, fmaxf(vb, vc))) + grow;
    if (cl > (float)(w - 1) || ch < 0.0f || rl > (float)(h - 1) || rh < 0.0f) return RasterBox{0, -1, 0, -1};  // off the image
    // (clamped as floats: the conversions are in range)
    return RasterBox{(int)fmaxf(rl, 0.0f), (int)fminf(rh, (float)(h - 1)), (int)fmaxf(cl, 0.0f), (int)fminf(ch, (float)(w - 1))};
}

__global__ __launch_bounds__(kRasterBlock) void raster_kernel(RasterLaunch L)
{
    const RasterView &V = L.v[blockIdx.y];
    const int f = blockIdx.x * kRasterBlock + threadIdx.x;
    const int h = L.h, w = L.w;
    unsigned long long *const keys = L.keys + (size_t)blockIdx.y * ((size_t)h * w);

    RasterTri T;
    RasterBox B{0, -1, 0, -1};
    if (f < L.m.nf) B = triangle_box(L.m, V, f, h, w, T);
    const int r0 = B.r0, r1 = B.r1, c0 = B.c0, c1 = B.c1;

    bool any = r1 >= r0 && c1 >= c0;
    const bool small = any && (r1 - r0) < kSmallBox && (c1 - c0) < kSmallBox;
    if (small) {
        for (int r = r0; r <= r1; ++r)
            for (int c = c0; c <= c1; ++c) test_pixel(V, T, r, c, L.near, (uint32_t)f, keys, w);
    }
    if (any && (r1 - r0 + 1) * (c1 - c0 + 1) > kDeferArea) {  // to the list, for raster_large_kernel; a full list: stays here
        const uint32_t slot = atomicAdd(L.count, 1u);
        if (slot < L.cap) {
            L.list_view[slot] = blockIdx.y;
            L.list_face[slot] = (uint32_t)f;
            any = false;
        }
    }

    // the boxes in between, one at a time by the whole wave
    const int lane = threadIdx.x & 63;
    const int ly = lane >> 3, lx = lane & 7;
    unsigned long long todo = __ballot(any && !small);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        RasterTri S;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            S.n0[k] = __shfl(T.n0[k], src);
            S.n1[k] = __shfl(T.n1[k], src);
            S.n2[k] = __shfl(T.n2[k], src);
        }
        S.det = __shfl(T.det, src);
        const int br0 = __shfl(r0, src), br1 = __shfl(r1, src), bc0 = __shfl(c0, src), bc1 = __shfl(c1, src);
        const uint32_t bf = (uint32_t)__shfl(f, src);
        for (int r = br0 + ly; r <= br1; r += 8)
            for (int c = bc0 + lx; c <= bc1; c += 8) test_pixel(V, S, r, c, L.near, bf, keys, w);
    }
}

// The listed (view, triangle) pairs, each cut into kStrips bands of rows; the waves of a fixed grid take the (pair, band)
// units in turn, 4 x 16 pixels at a time.  Every lane of a wave repeats the triangle's setup (the same bits as in raster_kernel).
__global__ __launch_bounds__(kRasterBlock) void raster_large_kernel(RasterLaunch L)
{
    const uint32_t count = *L.count < L.cap ? *L.count : L.cap;
    const uint32_t waves = gridDim.x * (kRasterBlock / 64);
    const uint32_t wave = blockIdx.x * (kRasterBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int ly = lane >> 4, lx = lane & 15;
    const int h = L.h, w = L.w;
    for (uint64_t u = wave; u < (uint64_t)count * kStrips; u += waves) {
        const uint32_t e = (uint32_t)(u / kStrips);
        const int j = (int)(u % kStrips);
        const uint32_t view = L.list_view[e], f = L.list_face[e];
        const RasterView &V = L.v[view];
        RasterTri T;
        const RasterBox B = triangle_box(L.m, V, (int)f, h, w, T);
        const int rows = B.r1 - B.r0 + 1;
        const int rs = B.r0 + (int)(((int64_t)rows * j) / kStrips), re = B.r0 + (int)(((int64_t)rows * (j + 1)) / kStrips) - 1;
        unsigned long long *const keys = L.keys + (size_t)view * ((size_t)h * w);
        for (int r = rs + ly; r <= re; r += 4)
            for (int c = B.c0 + lx; c <= B.c1; c += 16) test_pixel(V, T, r, c, L.near, f, keys, w);
    }
}

__global__ __launch_bounds__(kRasterBlock) void raster_resolve_kernel(const unsigned long long *keys, uint32_t total, float *depth, int *face)
{
    const uint32_t i = blockIdx.x * kRasterBlock + threadIdx.x;
    if (i >= total) return;
    const unsigned long long k = keys[i];
    const bool hit = k != ~0ULL;
    depth[i] = hit ? __uint_as_float((uint32_t)(k >> 32)) : 0.0f;
    face[i] = hit ? (int)(uint32_t)k : -1;
}

struct RasterAttrLaunch {
    RasterMesh m;
    const int *face;
    const uint8_t *face_labels;
    const uint32_t *vertex_rgba;
    uint8_t *labels;
    uint32_t *rgba;
    int h, w;
    RasterView v[OJF_RASTER_MAX_VIEWS];
};

__global__ __launch_bounds__(kRasterBlock) void raster_attr_kernel(RasterAttrLaunch L)
{
    const uint32_t i = blockIdx.x * kRasterBlock + threadIdx.x;  // pixel of view blockIdx.y
    if (i >= (uint32_t)(L.h * L.w)) return;
    const RasterView &V = L.v[blockIdx.y];
    const size_t pix = (size_t)blockIdx.y * (size_t)(L.h * L.w) + i;
    const int f = L.face[pix];
    uint8_t label = 0;
    uint32_t out = 0;
    float a[3], b[3], c[3];
    int idx[3];
    RasterTri T;
    if ((unsigned)f < (unsigned)L.m.nf && setup_triangle(L.m, V, f, a, b, c, T, idx)) {
        if (L.labels) label = L.face_labels[f];
        if (L.rgba) {
            float e[3], S;
            edge_values(V, T, (int)(i / (uint32_t)L.w), (int)(i % (uint32_t)L.w), e, S);
            const float l0 = e[0] / S, l1 = e[1] / S, l2 = e[2] / S;
            const uint32_t C0 = L.vertex_rgba[idx[0]], C1 = L.vertex_rgba[idx[1]], C2 = L.vertex_rgba[idx[2]];
            out = 0xff000000u;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float ck = (l0 * (float)((C0 >> (8 * k)) & 0xffu) + l1 * (float)((C1 >> (8 * k)) & 0xffu)) +
                                 l2 * (float)((C2 >> (8 * k)) & 0xffu);
                const float m = fminf(fmaxf(floorf(ck + 0.5f), 0.0f), 255.0f);  // (maxNum: a NaN gives 0)
                out |= (uint32_t)(int)m << (8 * k);
            }
        }
    }
    if (L.labels) L.labels[pix] = label;
    if (L.rgba) L.rgba[pix] = out;
}

// What both entry points ask of their mesh, images and cameras; 0 or refuse(who, ...).
static int check_raster(const char *who, const float *vertices, int nv, const int *faces, int nf, int n, const double *K,
                        const double *E, int h, int w)
{
    if (!vertices || !faces || !K || !E) return refuse(who, "null pointer argument");
    if (n < 1 || n > OJF_RASTER_MAX_VIEWS) return refuse(who, "n must be 1..OJF_RASTER_MAX_VIEWS views");
    if (nv < 1 || nf < 1) return refuse(who, "non-positive mesh size (nv, nf)");
    if ((int64_t)nf * 3 > 0x7fffffffLL || (int64_t)nv * 3 > 0x7fffffffLL) return refuse(who, "mesh too large");
    if (h <= 0 || w <= 0) return refuse(who, "non-positive image size");
    if ((int64_t)n * h * w > 0x7fffffffLL || h > (1 << 24) || w > (1 << 24)) return refuse(who, "images too large");
    if (!all_finite(K, 9 * n) || !all_finite(E, 12 * n)) return refuse(who, "non-finite K or E");
    for (int v = 0; v < n; ++v) {
        const double *Kv = K + 9 * v;
        if (Kv[1] != 0.0 || Kv[3] != 0.0 || Kv[6] != 0.0 || Kv[7] != 0.0 || Kv[8] != 1.0)
            return refuse(who, "K must be a pinhole matrix [fx 0 cx; 0 fy cy; 0 0 1]");
        if ((float)Kv[0] == 0.0f || (float)Kv[4] == 0.0f || !std::isfinite((float)Kv[0]) || !std::isfinite((float)Kv[4]))
            return refuse(who, "K: fx and fy must be non-zero and finite as floats");
    }
    if (((uintptr_t)vertices & 3) || ((uintptr_t)faces & 3)) return refuse(who, "vertices_dev and faces_dev must be 4-byte aligned");
    return 0;
}

static void make_raster_view(const double *Kv, const double *Ev, int h, int w, RasterView &V)
{
    for (int m = 0; m < 3; ++m) {
        for (int a = 0; a < 3; ++a) V.R[3 * m + a] = (float)Ev[4 * m + a];
        V.t[m] = (float)Ev[4 * m + 3];
    }
    V.fx = (float)Kv[0]; V.fy = (float)Kv[4]; V.cx = (float)Kv[2]; V.cy = (float)Kv[5];
    // F of the header (f64; only the box depends on it, never an output bit)
    const double rx = std::fmax(std::fabs(Kv[2]), std::fabs((double)(w - 1) - Kv[2])) / std::fabs(Kv[0]);
    const double ry = std::fmax(std::fabs(Kv[5]), std::fabs((double)(h - 1) - Kv[5])) / std::fabs(Kv[4]);
    const double F = std::fmax(std::fabs(Kv[0]), std::fabs(Kv[4])) * (1.0 + rx * rx + ry * ry);
    V.slack = (float)(4.0 * F / 16777216.0);
}

}  // namespace ojf

OJF_API int ojf_rasterize(const float *vertices, int nv, const int *faces, int nf, int n, const double *K, const double *E, int h,
                          int w, float near, uint64_t *keys, float *depth, int *face, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_rasterize";
    if (!keys || !depth || !face) return refuse(who, "null pointer argument");
    if (int rc = check_raster(who, vertices, nv, faces, nf, n, K, E, h, w)) return rc;
    if (!(near >= 0.0f) || !std::isfinite(near)) return refuse(who, "near must be >= 0 and finite");
    if (((uintptr_t)keys & 7) || ((uintptr_t)depth & 3) || ((uintptr_t)face & 3))
        return refuse(who, "keys_dev must be 8-byte, depth_dev and face_dev 4-byte aligned");
    RasterLaunch L;
    L.m = RasterMesh{vertices, faces, nv, nf};
    L.keys = reinterpret_cast<unsigned long long *>(keys);
    L.h = h; L.w = w; L.near = near;
    for (int v = 0; v < n; ++v) make_raster_view(K + 9 * v, E + 12 * v, h, w, L.v[v]);
    const size_t total = (size_t)n * h * w;
    // depth_dev and face_dev hold the list until raster_resolve_kernel writes them: word 0 of depth_dev its length, entry i
    // (view, face) in word 1 + i of depth_dev and of face_dev
    L.count = reinterpret_cast<uint32_t *>(depth);
    L.list_view = L.count + 1;
    L.list_face = reinterpret_cast<uint32_t *>(face) + 1;
    L.cap = (uint32_t)(total - 1);
    OJF_HIP(hipMemsetAsync(keys, 0xff, total * sizeof(uint64_t), as_stream(stream)));
    OJF_HIP(hipMemsetAsync(L.count, 0, sizeof(uint32_t), as_stream(stream)));
    const uint32_t tri_blocks = ((uint32_t)nf + kRasterBlock - 1) / kRasterBlock;
    hipLaunchKernelGGL(raster_kernel, dim3(tri_blocks, n), dim3(kRasterBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    hipLaunchKernelGGL(raster_large_kernel, dim3(kLargeBlocks), dim3(kRasterBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    const uint32_t blocks = (uint32_t)((total + kRasterBlock - 1) / kRasterBlock);
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(blocks), dim3(kRasterBlock), 0, as_stream(stream), L.keys, (uint32_t)total, depth, face);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_rasterize_attributes(const float *vertices, int nv, const int *faces, int nf, int n, const double *K,
                                     const double *E, int h, int w, const int *face, const uint8_t *face_labels,
                                     const uint8_t *vertex_rgba, uint8_t *labels, uint8_t *rgba, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_rasterize_attributes";
    if (!face) return refuse(who, "null pointer argument");
    if (int rc = check_raster(who, vertices, nv, faces, nf, n, K, E, h, w)) return rc;
    if (!labels && !rgba) return refuse(who, "neither labels_dev nor rgba_dev: nothing to do");
    if ((labels != nullptr) != (face_labels != nullptr)) return refuse(who, "face_labels_dev and labels_dev are both set or both NULL");
    if ((rgba != nullptr) != (vertex_rgba != nullptr)) return refuse(who, "vertex_rgba_dev and rgba_dev are both set or both NULL");
    if (((uintptr_t)face & 3) || ((uintptr_t)vertex_rgba & 3) || ((uintptr_t)rgba & 3))
        return refuse(who, "face_dev, vertex_rgba_dev and rgba_dev must be 4-byte aligned");
    RasterAttrLaunch L;
    L.m = RasterMesh{vertices, faces, nv, nf};
    L.face = face;
    L.face_labels = face_labels;
    L.vertex_rgba = reinterpret_cast<const uint32_t *>(vertex_rgba);
    L.labels = labels;
    L.rgba = reinterpret_cast<uint32_t *>(rgba);
    L.h = h; L.w = w;
    for (int v = 0; v < n; ++v) make_raster_view(K + 9 * v, E + 12 * v, h, w, L.v[v]);
    const uint32_t blocks = ((uint32_t)(h * w) + kRasterBlock - 1) / kRasterBlock;
    hipLaunchKernelGGL(raster_attr_kernel, dim3(blocks, n), dim3(kRasterBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    return 0;
}
