// MESH DISTANCE: the exact Euclidean distance from every voxel centre of a box to a triangle mesh, within a band, with the
// nearest face - the way from a mesh to a Euclidean TSDF, to label grids that need no cameras and to distance-to-surface
// volumes.  (The reference voxelises the mesh and runs a distance transform over the grid; neither is used here.)  Own
// definition; tests/mesh_distance_ref.py restates it in numpy, every voxel against every triangle, and the GPU tests pin
// the kernels to it bit for bit.
//
// Normative definition.  All device arithmetic below is fp32 with every product, sum and division rounded on its own (the
// build's -ffp-contract=off and correctly rounded division and square root).
//   u.v = (u0·v0 + u1·v1) + u2·v2;   u×v = (u1·v2 - u2·v1, u2·v0 - u0·v2, u0·v1 - u1·v0);   u - v component-wise.
//
// Inputs: vertices f32 [nv][3], faces i32 [nf][3]; the box origin f64[3] (host), resolution, X, Y, Z; band > 0 (metres).
//   voxel centre:  p_m = (float)(origin_m + ((double)i_m + 0.5)·resolution)  (f64 product, f64 sum, one rounding to fp32):
//       the frame of extract, integrate, render and ojf_fuse_projective.
//   triangle (a, b, c) in face order, v_0 = a, v_1 = b, v_2 = c:
//       e_0 = b - a, e_1 = c - b, e_2 = a - c;   n = e_0 × (c - a);   nn = n.n;   ee_k = e_k.e_k;
//       w_k = p - v_k;   h = w_0.n;   f_k = (e_k × w_k).n.
//   segment candidate k = 0, 1, 2:  t_k = 0 when ee_k == 0, else (w_k.e_k) / ee_k clamped to [0, 1] (t < 0 -> 0, then
//       t > 1 -> 1);  r_k = w_k - t_k·e_k component-wise (the product rounded, then the difference);  s_k = r_k.r_k.
//   plane candidate: counts when nn > 0 and f_0 >= 0 and f_1 >= 0 and f_2 >= 0;  s_3 = (h·h) / nn.
//   d² and the closest feature:  best = s_0;  s_1 replaces it when s_1 < best;  then s_2 when s_2 < best;  then the plane
//       candidate when it counts and s_3 <= best.  (A NaN never replaces anything.)  d² = best; the candidate that holds
//       it last is the winner.  A zero-area triangle is its three edges; nothing divides by zero.
//   skipped faces: an index outside [0, nv), or a vertex with a non-finite coordinate.
//   band² = (float)band·(float)band.  A face reaches a voxel when d² <= band² (false for a NaN).
//   key = (bits(d²) << 32) | face, as a u64; a voxel keeps the minimum key over the faces that reach it: the nearest face,
//       ties to the lower index (d² >= +0, so the bits order as the values do).
//   distance f32 [X,Y,Z] = sqrtf(d²) of the kept key, +inf where no face reaches;  face i32 [X,Y,Z]: its face, -1 there.
// The outputs are a function of (mesh, box, band) alone: not of the binning below, nor of the order of any list.
//
// Sign (ojf_mesh_distance_sign), per voxel with f = face[voxel] >= 0: the candidates of face f are formed again as above
//   and the winner names the closest feature:  the plane candidate - the face, s = h;  segment k with t_k == 0 - vertex
//   v_k, N = vertex_normals[index of v_k];  t_k == 1 - vertex v_(k+1 mod 3);  else edge k, N = edge_normals[face_edges[f][k]];
//   for a vertex or an edge s = r_k.N.  signed = distance where s >= 0, else -distance; +inf where face < 0 (and for a face
//   entry >= nf or a skipped face).  The normals are angle-weighted pseudonormals (Baerentzen & Aanaes 2005) that the
//   caller prepares: positive outside a closed, consistently outward-wound, non-self-intersecting mesh - and only there.
//
// Shape.  Bucket first, then gather; no float atomics.  The box is cut into bricks of 8 x 8 x 8 voxels.
//   bin (mesh_bin_kernel, twice: to count, then to fill): one lane per triangle takes the box of voxel indices whose
//     centres lie inside the triangle's bounding box dilated by R (below), clamped to the volume, and from it a box of
//     bricks.  Up to 8 bricks the lane visits them itself; more (a wall that spans thousands of bricks) are taken one
//     triangle at a time by the whole wave (a loop over __ballot, the triangle re-read from its lane), which also drops the
//     bricks whose centre is farther from the triangle's plane than R + the brick's half diagonal (f64).  Counting adds 1
//     to the brick's u32 counter (integer atomicAdd); mesh_pairs_scan_kernel turns counts into exclusive offsets and the total
//     number of (triangle, brick) pairs; filling writes the face index at an atomic cursor.  The order inside a brick's
//     list is whatever the atomics give; it shows in no output, because the minimum of the keys does not depend on it.
//   distance (mesh_distance_kernel): one workgroup of 256 lanes per brick, each lane owns two voxels (x and x + 4) and keeps
//     their minimum keys in registers.  The brick's list is staged through LDS kChunk triangles at a time: lane j of the
//     first kChunk fetches triangle j's vertices and forms e_k, n, nn, ee_k once for the 512 voxels, and the triangle's
//     bounding box widened by sv (below).  A voxel first takes q, its squared distance to that box (a dozen operations),
//     and skips the triangle when q > min(band², the d² it already holds): such a triangle can neither reach the voxel
//     nor replace its key - branch and bound, with the same bits as meeting every triangle.  A wave whose 64 voxels all
//     skip pays only for q.  Plain stores; a brick with an empty list writes +inf / -1.
//   The number of pairs is not known before the count: the entry point is called with capacity 0 to get it, then again with
//     a list of that capacity (the idiom of ojf_mesh_extract).
//
// R and why the bins lose nothing.  A face reaches a voxel when the *rounded* d² <= band².  Every quantity above is a sum
// of a few products of differences of coordinates; with G the largest magnitude of a coordinate involved (the triangle's
// vertices and the voxel centres of the box), D the triangle's extent (the sum of the three sides of its bounding box) and
// eps = 2^-24, the rounded distance differs from the distance to the exact triangle by a small multiple of eps·(G + D +
// band): the centre's own rounding is at most eps·G, w_k has one rounding of a value <= D + band, t_k·e_k and r_k a few
// more of values <= D, the dot products a relative 3 eps.  The plane candidate is accepted by the rounded f_k, whose error
// eps·|e_k||w_k||n| moves the edge's line by about eps·|w_k| in the plane, whatever the triangle's shape.  So a voxel
// that a face reaches lies within band + c·eps·(G + D + band) of the exact triangle, with c of the order of ten, hence
// within that of its bounding box on every axis.  R = band + 2^-18·(G + D + band): c = 64.  The index box is computed in
// f64, whose own rounding is nine orders of magnitude below that slack.  The distance kernel's bound works in fp32 with
// sv = 2^-16·((G + D) + band), c = 256: the box is [lo - sv, hi + sv], x_m = max(lo_m - sv - p_m, p_m - hi_m - sv, 0) and
// q = x_0·x_0 + (x_1·x_1 + x_2·x_2).  Shrinking every non-zero excess by sv shortens the vector of excesses by at least
// sv / sqrt(3) (its largest component is at least that share of its length), so sqrt(q) <= (the distance to the exact
// bounding box) - 147·eps·(G + D + band), of which the roundings of lo - sv, hi + sv and q take a few units; the rounded
// d² of the triangle is then strictly above q, and q > L for a limit L (band², or a d² the voxel already holds) means
// that d² > L: the triangle neither reaches the voxel nor wins or ties its key.  This is reasoning about magnitudes,
// not a proof; the GPU tests compare with the bin-free, bound-free reference on meshes with zero-area, sliver, far-away
// and box-spanning triangles, at bands from a fraction of a voxel to more than the box.
#include "ojf_blocks.h"

namespace ojf {

constexpr int kBrick = 8;           // voxels per brick side
constexpr int kDistBlock = 256;     // lanes of mesh_distance_kernel: two voxels each
constexpr int kChunk = 128;         // triangles staged through LDS at a time
constexpr int kTriWords = 32;       // words of one staged triangle (TriPrep, the face index, the widened bounding box)
constexpr int kBinBlock = 256;
constexpr int kLaneBricks = 8;      // brick boxes up to this many bricks are visited by the triangle's own lane
constexpr double kSlack = 1.0 / 262144.0;  // 2^-18 (the header's c·eps)
constexpr float kVoxelSlack = 1.0f / 65536.0f;  // 2^-16: the header's sv over (G + D + band)
constexpr double kBrickRadius = 6.07;      // > 3.5·sqrt(3): from a brick's centre to its farthest voxel centre, in voxels

struct MeshBox {  // by value in the kernel arguments
    double origin[3];
    double res;
    double gmax;  // largest magnitude of a voxel-centre coordinate of the box
    int X, Y, Z;
    int nbx, nby, nbz;
};

struct MeshRef {
    const float *vertices;
    const int *faces;
    int nv, nf;
};

struct TriPrep {  // what the distance needs of one triangle (the header's names)
    float a[3], b[3], c[3];
    float e0[3], e1[3], e2[3];
    float n[3];
    float nn;
    float ee[3];
};

// Face f of the mesh: false for a skipped face, else its vertices and their indices.
__device__ __forceinline__ bool load_face(const MeshRef &M, int f, float P[3][3], int idx[3])
{
    idx[0] = M.faces[3 * (size_t)f]; idx[1] = M.faces[3 * (size_t)f + 1]; idx[2] = M.faces[3 * (size_t)f + 2];
    if ((unsigned)idx[0] >= (unsigned)M.nv || (unsigned)idx[1] >= (unsigned)M.nv || (unsigned)idx[2] >= (unsigned)M.nv) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) P[i][k] = M.vertices[3 * (size_t)idx[i] + k];
        if (!finite3(P[i])) return false;
    }
    return true;
}

__device__ __forceinline__ void prepare_triangle(const float P[3][3], TriPrep &T)
{
    float ac[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        T.a[m] = P[0][m]; T.b[m] = P[1][m]; T.c[m] = P[2][m];
        T.e0[m] = P[1][m] - P[0][m];
        T.e1[m] = P[2][m] - P[1][m];
        T.e2[m] = P[0][m] - P[2][m];
        ac[m] = P[2][m] - P[0][m];
    }
    cross3(T.e0, ac, T.n);
    T.nn = dot3(T.n, T.n);
    T.ee[0] = dot3(T.e0, T.e0);
    T.ee[1] = dot3(T.e1, T.e1);
    T.ee[2] = dot3(T.e2, T.e2);
}

// segment candidate: t, r = w - t·e and s = r.r
__device__ __forceinline__ float segment_candidate(const float w[3], const float e[3], float ee, float &t, float r[3])
{
    t = 0.0f;
    if (ee > 0.0f) {
        t = dot3(w, e) / ee;
        t = t < 0.0f ? 0.0f : t;
        t = t > 1.0f ? 1.0f : t;
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) r[m] = w[m] - t * e[m];
    return dot3(r, r);
}

struct Closest {  // the winner of the header's candidate order (the sign needs more than d²)
    float d2;
    int feature;  // 0..2: segment k, 3: the plane
    float t, r[3], h;
};

__device__ __forceinline__ void closest_feature(const float p[3], const TriPrep &T, Closest &C)
{
    float w0[3], w1[3], w2[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        w0[m] = p[m] - T.a[m];
        w1[m] = p[m] - T.b[m];
        w2[m] = p[m] - T.c[m];
    }
    float t, r[3];
    C.d2 = segment_candidate(w0, T.e0, T.ee[0], C.t, C.r);
    C.feature = 0;
    float s = segment_candidate(w1, T.e1, T.ee[1], t, r);
    if (s < C.d2) { C.d2 = s; C.feature = 1; C.t = t; C.r[0] = r[0]; C.r[1] = r[1]; C.r[2] = r[2]; }
    s = segment_candidate(w2, T.e2, T.ee[2], t, r);
    if (s < C.d2) { C.d2 = s; C.feature = 2; C.t = t; C.r[0] = r[0]; C.r[1] = r[1]; C.r[2] = r[2]; }
    C.h = dot3(w0, T.n);
    if (T.nn > 0.0f) {
        float x[3];
        cross3(T.e0, w0, x);
        const float f0 = dot3(x, T.n);
        cross3(T.e1, w1, x);
        const float f1 = dot3(x, T.n);
        cross3(T.e2, w2, x);
        const float f2 = dot3(x, T.n);
        if (f0 >= 0.0f && f1 >= 0.0f && f2 >= 0.0f) {
            const float s3 = (C.h * C.h) / T.nn;
            if (s3 <= C.d2) { C.d2 = s3; C.feature = 3; }
        }
    }
}

// d² alone (the same operations as closest_feature; what the distance kernel runs per voxel and triangle)
__device__ __forceinline__ float triangle_d2(const float p[3], const TriPrep &T)
{
    Closest C;
    closest_feature(p, T, C);
    return C.d2;
}

__device__ __forceinline__ float voxel_centre(const MeshBox &B, int m, int i) { return (float)(B.origin[m] + ((double)i + 0.5) * B.res); }

// ---- bin -----------------------------------------------------------------------------------------------------------------
struct BinLaunch {
    MeshRef m;
    MeshBox box;
    double band;         // (double)(float)band
    uint32_t *counts;    // [bricks]
    uint32_t *cursor;    // [bricks], when filling
    uint32_t *pairs;     // the lists, when filling
    uint32_t cap;
};

struct BrickBox {
    int b0[3], b1[3];  // bricks, inclusive; b1[0] < b0[0]: empty
    double R;
    double a[3], n[3], nlen;  // the plane, f64 (nlen 0: no plane test)
};

// The brick box of face f (the header's R); empty for a skipped face or one that reaches no voxel of the volume.
__device__ __forceinline__ void brick_box(const BinLaunch &L, int f, BrickBox &Q)
{
    Q.b0[0] = 0; Q.b1[0] = -1;
    float P[3][3];
    int idx[3];
    if (!load_face(L.m, f, P, idx)) return;
    double lo[3], hi[3], D = 0.0, G = L.box.gmax;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        lo[m] = (double)fminf(P[0][m], fminf(P[1][m], P[2][m]));
        hi[m] = (double)fmaxf(P[0][m], fmaxf(P[1][m], P[2][m]));
        D += hi[m] - lo[m];
        G = fmax(G, fmax(fabs(lo[m]), fabs(hi[m])));
    }
    const double R = L.band + kSlack * ((G + D) + L.band);
    const int dims[3] = {L.box.X, L.box.Y, L.box.Z};
    int b0[3], b1[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        // voxel i's centre is origin + (i + 0.5)·res: inside [lo - R, hi + R] for ceil(x0) <= i <= floor(x1)
        double i0 = ceil(((lo[m] - R) - L.box.origin[m]) / L.box.res - 0.5);
        double i1 = floor(((hi[m] + R) - L.box.origin[m]) / L.box.res - 0.5);
        i0 = fmax(i0, 0.0);
        i1 = fmin(i1, (double)(dims[m] - 1));
        if (!(i0 <= i1)) return;  // (clamped as doubles: the conversions are in range)
        b0[m] = (int)i0 / kBrick;
        b1[m] = (int)i1 / kBrick;
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) { Q.b0[m] = b0[m]; Q.b1[m] = b1[m]; }
    Q.R = R;
    double e0[3], ac[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        Q.a[m] = (double)P[0][m];
        e0[m] = (double)P[1][m] - (double)P[0][m];
        ac[m] = (double)P[2][m] - (double)P[0][m];
    }
    Q.n[0] = e0[1] * ac[2] - e0[2] * ac[1];
    Q.n[1] = e0[2] * ac[0] - e0[0] * ac[2];
    Q.n[2] = e0[0] * ac[1] - e0[1] * ac[0];
    Q.nlen = sqrt((Q.n[0] * Q.n[0] + Q.n[1] * Q.n[1]) + Q.n[2] * Q.n[2]);
    if (!(Q.nlen > 0.0 && Q.nlen < (double)INFINITY)) Q.nlen = 0.0;
}

// false when every voxel centre of brick (bx, by, bz) is farther than R from the triangle's plane
__device__ __forceinline__ bool brick_near_plane(const MeshBox &B, const BrickBox &Q, int bx, int by, int bz)
{
    if (Q.nlen == 0.0) return true;
    const double c0 = B.origin[0] + (double)(kBrick * bx + kBrick / 2) * B.res - Q.a[0];
    const double c1 = B.origin[1] + (double)(kBrick * by + kBrick / 2) * B.res - Q.a[1];
    const double c2 = B.origin[2] + (double)(kBrick * bz + kBrick / 2) * B.res - Q.a[2];
    const double dist = fabs((c0 * Q.n[0] + c1 * Q.n[1]) + c2 * Q.n[2]) / Q.nlen;
    return !(dist > Q.R + kBrickRadius * B.res);  // (a NaN keeps the brick)
}

template <bool kFill>
__device__ __forceinline__ void bin_pair(const BinLaunch &L, int bx, int by, int bz, uint32_t f)
{
    const uint32_t b = ((uint32_t)bx * (uint32_t)L.box.nby + (uint32_t)by) * (uint32_t)L.box.nbz + (uint32_t)bz;
    if (kFill) {
        const uint32_t slot = atomicAdd(L.cursor + b, 1u);
        if (slot < L.cap) L.pairs[slot] = f;
    } else {
        atomicAdd(L.counts + b, 1u);
    }
}

template <bool kFill>
__global__ __launch_bounds__(kBinBlock) void mesh_bin_kernel(BinLaunch L)
{
    const int f = blockIdx.x * kBinBlock + threadIdx.x;
    BrickBox Q;
    Q.b0[0] = 0; Q.b1[0] = -1;
    if (f < L.m.nf) brick_box(L, f, Q);
    const bool any = Q.b1[0] >= Q.b0[0];
    int64_t bricks = 0;
    if (any) bricks = (int64_t)(Q.b1[0] - Q.b0[0] + 1) * (Q.b1[1] - Q.b0[1] + 1) * (Q.b1[2] - Q.b0[2] + 1);
    const bool small = any && bricks <= kLaneBricks;
    if (small) {
        for (int bx = Q.b0[0]; bx <= Q.b1[0]; ++bx)
            for (int by = Q.b0[1]; by <= Q.b1[1]; ++by)
                for (int bz = Q.b0[2]; bz <= Q.b1[2]; ++bz) bin_pair<kFill>(L, bx, by, bz, (uint32_t)f);
    }
    // the larger boxes, one at a time by the whole wave; every lane repeats the triangle's setup (the same bits)
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(any && !small);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int sf = __shfl(f, src);
        BrickBox S;
        brick_box(L, sf, S);
        const int ny = S.b1[1] - S.b0[1] + 1, nz = S.b1[2] - S.b0[2] + 1;
        const int64_t total = (int64_t)(S.b1[0] - S.b0[0] + 1) * ny * nz;
        for (int64_t u = lane; u < total; u += 64) {
            const int bz = S.b0[2] + (int)(u % nz);
            const int by = S.b0[1] + (int)((u / nz) % ny);
            const int bx = S.b0[0] + (int)(u / ((int64_t)nz * ny));
            if (brick_near_plane(L.box, S, bx, by, bz)) bin_pair<kFill>(L, bx, by, bz, (uint32_t)sf);
        }
    }
}

// counts -> exclusive offsets (and the fill's cursors), the total to total_ws and *count_out.  Sums are u64, offsets u32: a
// total of 2^32 pairs or more wraps them (the entry point's callers see the total and refuse; the lists stay inside cap).
__global__ __launch_bounds__(kScanBlock) void mesh_pairs_scan_kernel(const uint32_t *counts, uint32_t nb, uint32_t *offsets,
                                                                     unsigned long long *total_ws, unsigned long long *count_out)
{
    const unsigned long long total = block_exclusive_scan<unsigned long long>(counts, offsets, nb);
    if (threadIdx.x == kScanBlock - 1) {
        *total_ws = total;
        if (count_out) *count_out = total;
    }
}

// ---- distance ------------------------------------------------------------------------------------------------------------
struct DistLaunch {
    MeshRef m;
    MeshBox box;
    float band, band2, gmax;
    const uint32_t *counts, *offsets, *pairs;
    uint32_t cap;
    float *distance;
    int *face;
};

__global__ __launch_bounds__(kDistBlock) void mesh_distance_kernel(DistLaunch L)
{
    __shared__ float tri[kTriWords][kChunk];  // [word][triangle]: lanes of a wave write neighbouring banks, reads are broadcasts
    const uint32_t b = blockIdx.x;
    const int bz = (int)(b % (uint32_t)L.box.nbz);
    const int by = (int)((b / (uint32_t)L.box.nbz) % (uint32_t)L.box.nby);
    const int bx = (int)(b / ((uint32_t)L.box.nbz * (uint32_t)L.box.nby));
    const int tid = threadIdx.x;
    const int x0 = kBrick * bx + (tid >> 6), x1 = x0 + kBrick / 2;
    const int y = kBrick * by + ((tid >> 3) & 7), z = kBrick * bz + (tid & 7);
    float p0[3], p1[3];
    p0[0] = voxel_centre(L.box, 0, x0);
    p1[0] = voxel_centre(L.box, 0, x1);
    p0[1] = p1[1] = voxel_centre(L.box, 1, y);
    p0[2] = p1[2] = voxel_centre(L.box, 2, z);
    unsigned long long key0 = ~0ULL, key1 = ~0ULL;
    float lim0 = L.band2, lim1 = L.band2;  // min(band², the d² of the key held)

    const uint32_t cnt = L.counts[b], off = L.offsets[b];
    for (uint32_t base = 0; base < cnt; base += kChunk) {
        const uint32_t n = cnt - base < (uint32_t)kChunk ? cnt - base : (uint32_t)kChunk;
        __syncthreads();  // the previous chunk has been read
        if ((uint32_t)tid < n) {
            const uint64_t slot = (uint64_t)off + base + (uint32_t)tid;
            int f = -1;
            float P[3][3];
            int idx[3];
            if (slot < L.cap) {
                const uint32_t e = L.pairs[slot];
                if (e < (uint32_t)L.m.nf && load_face(L.m, (int)e, P, idx)) f = (int)e;
            }
            if (f >= 0) {
                TriPrep T;
                prepare_triangle(P, T);
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    tri[m][tid] = T.a[m]; tri[3 + m][tid] = T.b[m]; tri[6 + m][tid] = T.c[m];
                    tri[9 + m][tid] = T.e0[m]; tri[12 + m][tid] = T.e1[m]; tri[15 + m][tid] = T.e2[m];
                    tri[18 + m][tid] = T.n[m];
                    tri[22 + m][tid] = T.ee[m];
                }
                tri[21][tid] = T.nn;
                // the widened bounding box (the header's sv); an overflow gives +-inf bounds, which exclude nothing
                float D = 0.0f, G = L.gmax, lo[3], hi[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    lo[m] = fminf(P[0][m], fminf(P[1][m], P[2][m]));
                    hi[m] = fmaxf(P[0][m], fmaxf(P[1][m], P[2][m]));
                    D += hi[m] - lo[m];
                    G = fmaxf(G, fmaxf(fabsf(lo[m]), fabsf(hi[m])));
                }
                const float sv = kVoxelSlack * ((G + D) + L.band);
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    tri[26 + m][tid] = lo[m] - sv;
                    tri[29 + m][tid] = hi[m] + sv;
                }
            }
            tri[25][tid] = __int_as_float(f);
        }
        __syncthreads();
        for (uint32_t j = 0; j < n; ++j) {
            const int f = __float_as_int(tri[25][j]);
            if (f < 0) continue;  // (the same for every lane)
            const float lx = tri[26][j], hx = tri[29][j];
            const float ey = fmaxf(fmaxf(tri[27][j] - p0[1], p0[1] - tri[30][j]), 0.0f);
            const float ez = fmaxf(fmaxf(tri[28][j] - p0[2], p0[2] - tri[31][j]), 0.0f);
            const float ex0 = fmaxf(fmaxf(lx - p0[0], p0[0] - hx), 0.0f), ex1 = fmaxf(fmaxf(lx - p1[0], p1[0] - hx), 0.0f);
            const float qyz = ey * ey + ez * ez;
            const bool in0 = !(ex0 * ex0 + qyz > lim0), in1 = !(ex1 * ex1 + qyz > lim1);  // (a NaN meets the triangle)
            if (!(in0 || in1)) continue;
            TriPrep T;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                T.a[m] = tri[m][j]; T.b[m] = tri[3 + m][j]; T.c[m] = tri[6 + m][j];
                T.e0[m] = tri[9 + m][j]; T.e1[m] = tri[12 + m][j]; T.e2[m] = tri[15 + m][j];
                T.n[m] = tri[18 + m][j];
                T.ee[m] = tri[22 + m][j];
            }
            T.nn = tri[21][j];
            const float d0 = in0 ? triangle_d2(p0, T) : INFINITY, d1 = in1 ? triangle_d2(p1, T) : INFINITY;
            if (d0 <= L.band2) {
                const unsigned long long k = ((unsigned long long)__float_as_uint(d0) << 32) | (uint32_t)f;
                key0 = k < key0 ? k : key0;
                lim0 = d0 < lim0 ? d0 : lim0;
            }
            if (d1 <= L.band2) {
                const unsigned long long k = ((unsigned long long)__float_as_uint(d1) << 32) | (uint32_t)f;
                key1 = k < key1 ? k : key1;
                lim1 = d1 < lim1 ? d1 : lim1;
            }
        }
    }
    if (y < L.box.Y && z < L.box.Z) {
        if (x0 < L.box.X) {
            const size_t v = ((size_t)x0 * L.box.Y + y) * L.box.Z + z;
            L.distance[v] = key0 != ~0ULL ? sqrtf(__uint_as_float((uint32_t)(key0 >> 32))) : INFINITY;
            L.face[v] = key0 != ~0ULL ? (int)(uint32_t)key0 : -1;
        }
        if (x1 < L.box.X) {
            const size_t v = ((size_t)x1 * L.box.Y + y) * L.box.Z + z;
            L.distance[v] = key1 != ~0ULL ? sqrtf(__uint_as_float((uint32_t)(key1 >> 32))) : INFINITY;
            L.face[v] = key1 != ~0ULL ? (int)(uint32_t)key1 : -1;
        }
    }
}

// ---- sign ----------------------------------------------------------------------------------------------------------------
struct SignLaunch {
    MeshRef m;
    MeshBox box;
    const float *distance;
    const int *face;
    const float *vertex_normals, *edge_normals;
    const int *face_edges;
    int ne;
    float *out;
};

__global__ __launch_bounds__(kDistBlock) void mesh_sign_kernel(SignLaunch L)
{
    const uint32_t v = blockIdx.x * kDistBlock + threadIdx.x;
    const uint32_t total = (uint32_t)L.box.X * (uint32_t)L.box.Y * (uint32_t)L.box.Z;
    if (v >= total) return;
    const int k = (int)(v % (uint32_t)L.box.Z);
    const int j = (int)((v / (uint32_t)L.box.Z) % (uint32_t)L.box.Y);
    const int i = (int)(v / ((uint32_t)L.box.Z * (uint32_t)L.box.Y));
    const int f = L.face[v];
    float out = INFINITY;
    float P[3][3];
    int idx[3];
    if ((unsigned)f < (unsigned)L.m.nf && load_face(L.m, f, P, idx)) {
        TriPrep T;
        prepare_triangle(P, T);
        const float p[3] = {voxel_centre(L.box, 0, i), voxel_centre(L.box, 1, j), voxel_centre(L.box, 2, k)};
        Closest C;
        closest_feature(p, T, C);
        float s = C.h;
        if (C.feature < 3) {
            const float *N = nullptr;
            if (C.t == 0.0f) {
                N = L.vertex_normals + 3 * (size_t)idx[C.feature];
            } else if (C.t == 1.0f) {
                N = L.vertex_normals + 3 * (size_t)idx[(C.feature + 1) % 3];
            } else {
                const int e = L.face_edges[3 * (size_t)f + C.feature];
                if ((unsigned)e < (unsigned)L.ne) N = L.edge_normals + 3 * (size_t)e;
            }
            const float Nv[3] = {N ? N[0] : 0.0f, N ? N[1] : 0.0f, N ? N[2] : 0.0f};  // (an edge index out of range: a zero normal)
            s = dot3(C.r, Nv);
        }
        const float d = L.distance[v];
        out = s >= 0.0f ? d : -d;
    }
    L.out[v] = out;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static int check_mesh_box(const char *who, const float *vertices, int nv, const int *faces, int nf, const double *origin, double res,
                          int X, int Y, int Z)
{
    if (!vertices || !faces || !origin) return refuse(who, "null pointer argument");
    if (nv < 1 || nf < 1) return refuse(who, "non-positive mesh size (nv, nf)");
    if ((int64_t)nf * 3 > 0x7fffffffLL || (int64_t)nv * 3 > 0x7fffffffLL) return refuse(who, "mesh too large");
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    if (!all_finite(origin, 3) || !std::isfinite(res)) return refuse(who, "non-finite origin or resolution");
    if (!(res > 0.0)) return refuse(who, "resolution must be > 0");
    if (((uintptr_t)vertices & 3) || ((uintptr_t)faces & 3)) return refuse(who, "vertices_dev and faces_dev must be 4-byte aligned");
    return 0;
}

static MeshBox make_mesh_box(const double *origin, double res, int X, int Y, int Z)
{
    MeshBox B;
    const int dims[3] = {X, Y, Z};
    B.gmax = 0.0;
    for (int m = 0; m < 3; ++m) {
        B.origin[m] = origin[m];
        B.gmax = std::fmax(B.gmax, std::fmax(std::fabs(origin[m]), std::fabs(origin[m] + (double)dims[m] * res)));
    }
    B.res = res;
    B.X = X; B.Y = Y; B.Z = Z;
    B.nbx = (X + kBrick - 1) / kBrick; B.nby = (Y + kBrick - 1) / kBrick; B.nbz = (Z + kBrick - 1) / kBrick;
    return B;
}

static size_t mesh_bricks(int X, int Y, int Z)
{
    return (size_t)((X + kBrick - 1) / kBrick) * (size_t)((Y + kBrick - 1) / kBrick) * (size_t)((Z + kBrick - 1) / kBrick);
}

}  // namespace ojf

OJF_API size_t ojf_mesh_distance_workspace_bytes(int X, int Y, int Z)
{
    if (!ojf::volume_size_ok(X, Y, Z)) return 0;
    // counts, offsets, cursors (u32 per brick), rounded up to 8 bytes; the total (u64)
    return ((3 * ojf::mesh_bricks(X, Y, Z) * sizeof(uint32_t) + 7) & ~(size_t)7) + sizeof(uint64_t);
}

OJF_API int ojf_mesh_distance(const float *vertices, int nv, const int *faces, int nf, const double *origin, double resolution, int X,
                              int Y, int Z, float band, int phases, void *workspace, size_t workspace_bytes, uint32_t *pairs,
                              uint32_t capacity, uint64_t *count, float *distance, int *face, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_mesh_distance";
    if (!workspace) return refuse(who, "null pointer argument");
    if (int rc = check_mesh_box(who, vertices, nv, faces, nf, origin, resolution, X, Y, Z)) return rc;
    if (!std::isfinite(band) || !(band > 0.0f)) return refuse(who, "band must be > 0 and finite");
    if (phases < 1 || phases > OJF_MESH_DISTANCE_ALL) return refuse(who, "phases must be a non-empty set of OJF_MESH_DISTANCE_* bits");
    if (capacity == 0 && (phases & (OJF_MESH_DISTANCE_FILL | OJF_MESH_DISTANCE_GATHER))) phases &= OJF_MESH_DISTANCE_BIN | OJF_MESH_DISTANCE_SCAN;
    if (capacity == 0 && phases == 0) return refuse(who, "capacity 0 runs the bin and scan phases only");
    const bool lists = (phases & (OJF_MESH_DISTANCE_FILL | OJF_MESH_DISTANCE_GATHER)) != 0;
    if (lists && !pairs) return refuse(who, "null pointer argument: pairs_dev with capacity > 0");
    if ((phases & OJF_MESH_DISTANCE_GATHER) && (!distance || !face)) return refuse(who, "null pointer argument: distance_dev, face_dev");
    if (workspace_bytes < ojf_mesh_distance_workspace_bytes(X, Y, Z)) return refuse(who, "workspace too small");
    if (((uintptr_t)workspace & 7) || ((uintptr_t)pairs & 3) || ((uintptr_t)count & 7) || ((uintptr_t)distance & 3) || ((uintptr_t)face & 3))
        return refuse(who, "workspace_dev and count_dev must be 8-byte, pairs_dev, distance_dev and face_dev 4-byte aligned");

    const MeshBox B = make_mesh_box(origin, resolution, X, Y, Z);
    const size_t nb = mesh_bricks(X, Y, Z);
    uint32_t *const counts = reinterpret_cast<uint32_t *>(workspace);
    uint32_t *const offsets = counts + nb, *const cursor = offsets + nb;
    unsigned long long *const total = reinterpret_cast<unsigned long long *>(
        reinterpret_cast<char *>(workspace) + ((3 * nb * sizeof(uint32_t) + 7) & ~(size_t)7));
    BinLaunch L;
    L.m = MeshRef{vertices, faces, nv, nf};
    L.box = B;
    L.band = (double)band;
    L.counts = counts; L.cursor = cursor; L.pairs = pairs; L.cap = capacity;
    const uint32_t tri_blocks = ((uint32_t)nf + kBinBlock - 1) / kBinBlock;
    hipStream_t s = as_stream(stream);
    if (phases & OJF_MESH_DISTANCE_BIN) {
        OJF_HIP(hipMemsetAsync(counts, 0, nb * sizeof(uint32_t), s));
        hipLaunchKernelGGL(mesh_bin_kernel<false>, dim3(tri_blocks), dim3(kBinBlock), 0, s, L);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_MESH_DISTANCE_SCAN) {
        hipLaunchKernelGGL(mesh_pairs_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, counts, (uint32_t)nb, offsets, total,
                           reinterpret_cast<unsigned long long *>(count));
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_MESH_DISTANCE_FILL) {
        OJF_HIP(hipMemcpyAsync(cursor, offsets, nb * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(mesh_bin_kernel<true>, dim3(tri_blocks), dim3(kBinBlock), 0, s, L);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_MESH_DISTANCE_GATHER) {
        DistLaunch D;
        D.m = L.m;
        D.box = B;
        D.band = band;
        D.band2 = band * band;
        D.gmax = (float)B.gmax;
        D.counts = counts; D.offsets = offsets; D.pairs = pairs; D.cap = capacity;
        D.distance = distance; D.face = face;
        hipLaunchKernelGGL(mesh_distance_kernel, dim3((uint32_t)nb), dim3(kDistBlock), 0, s, D);
        OJF_HIP(hipGetLastError());
    }
    return 0;
}

OJF_API int ojf_mesh_distance_sign(const float *vertices, int nv, const int *faces, int nf, const double *origin, double resolution,
                                   int X, int Y, int Z, const float *distance, const int *face, const float *vertex_normals,
                                   const float *edge_normals, int ne, const int *face_edges, float *signed_out, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_mesh_distance_sign";
    if (!distance || !face || !vertex_normals || !edge_normals || !face_edges || !signed_out) return refuse(who, "null pointer argument");
    if (int rc = check_mesh_box(who, vertices, nv, faces, nf, origin, resolution, X, Y, Z)) return rc;
    if (ne < 1 || (int64_t)ne * 3 > 0x7fffffffLL) return refuse(who, "ne must be >= 1 (and 3·ne < 2^31)");
    if (((uintptr_t)distance & 3) || ((uintptr_t)face & 3) || ((uintptr_t)vertex_normals & 3) || ((uintptr_t)edge_normals & 3) ||
        ((uintptr_t)face_edges & 3) || ((uintptr_t)signed_out & 3))
        return refuse(who, "device arrays must be 4-byte aligned");
    SignLaunch L;
    L.m = MeshRef{vertices, faces, nv, nf};
    L.box = make_mesh_box(origin, resolution, X, Y, Z);
    L.distance = distance; L.face = face;
    L.vertex_normals = vertex_normals; L.edge_normals = edge_normals; L.face_edges = face_edges; L.ne = ne;
    L.out = signed_out;
    const uint32_t total = (uint32_t)X * (uint32_t)Y * (uint32_t)Z;
    hipLaunchKernelGGL(mesh_sign_kernel, dim3((total + kDistBlock - 1) / kDistBlock), dim3(kDistBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    return 0;
}
