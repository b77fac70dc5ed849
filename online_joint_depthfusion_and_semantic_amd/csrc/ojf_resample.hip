// RESAMPLE: a fused scene read through a rigid transform into another box - re-box (the box follows the camera), resample
// (another resolution) and merge (two fused sessions of one room) are one operator: every destination voxel gathers the
// trilinear mean of the observed source voxels around the point its centre maps to.  Own definition (the reference has no
// counterpart); tests/resample_ref.py restates it in numpy and the GPU tests pin the kernels to it bit for bit.
//
// Frame: the one ojf_render.hip states - voxel (i,j,k) has its centre at origin + (i+0.5, j+0.5, k+0.5)·res; index
// coordinates g put voxel (i,j,k) at g = (i,j,k), as in the colour sample of ojf_color.hip.
//
// Normative definition.
// Host (f64, resample.py): the destination box is origin_d, res_d, N_d, the source box origin_s, res_s, N_s; a rigid [R|t]
//     maps destination-world points to source-world points, x_s = R·x_d + t.  M = R·res_d/res_s and
//     c = (R·(origin_d + 0.5·res_d·1) + t - origin_s)/res_s - 0.5 come to the C ABI as f64 and are rounded once to fp32 here
//     (ojf_volume_filter's rule for its threshold).
// Device: all arithmetic is fp32 with every product, sum and division rounded on its own (the build's -ffp-contract=off
//     and correctly rounded division); fp16 conversions round to nearest even; min is IEEE minNum.  Per destination voxel
//     (i,j,k):
//     1. g_a = ((M[a][0]·i + M[a][1]·j) + M[a][2]·k) + c[a].
//     2. if any g_a is non-finite, < -1 or > N_s,a (float comparisons, before any conversion to int): no corner counts.
//        Else i0_a = floor(g_a), f_a = g_a - i0_a.
//     3. over the corners 000..111 (bits x, y, z, in that order): tw = (wx·wy)·wz with w_axis = (1 - f) or f.
//     4. a corner counts iff it lies inside the source grid, tw > 0 and it is observed: float(W_c) > 0 in the source weight
//        volume; without a weight volume (ground truth) every in-grid corner is observed.  A corner that does not count is
//        never loaded.
//     5. in corner order over the counting corners: ws += tw, acc += tw·float(T_c), accW += tw·float(W_c); ws and accW
//        start at 0, acc at -0, the identity of IEEE addition (0 + (-0) is +0; -0 + x is x for every x): the first term
//        enters the sum unchanged, so a source value of -0 that is copied stays -0.
//     6. the voxel is covered iff ws >= 0.5; then T' = half(acc/ws), W' = half(accW/ws); a covered voxel whose W' is +0
//        counts as uncovered.
//     7. labels (id and score volumes given): the counting corner with the largest tw, the first in corner order on a tie,
//        gives id' and the bits of score'.
//     8. records ([X,Y,Z,S] with the weight in channel Cw: colour S = 4, Cw = 3; class distributions S = record_size(C),
//        Cw = C): observed means float(rec_c[Cw]) > 0; every channel k < Cw takes half(acc_k/ws), channel Cw takes
//        half(accW/ws); channels above Cw are never read or written.
//   Replace mode: every destination voxel is written once - covered: T', W', id', score' (or the record); uncovered:
//     T = init_value, W = 0, id = 0, score = 0 (or record channels 0..Cw = 0).
//   Merge mode: an uncovered voxel leaves the destination untouched.  Covered, with w0 = float(W_d), w1 = float(W'):
//     T = T' if w0 == 0, else half((w0·float(T_d) + w1·float(T'))/(w0 + w1));  W = half(min(w0 + w1, max_weight));  id and
//     score are replaced iff float(score') > float(score_d) (step 6 of ojf_fuse_projective); records: the same running mean
//     per channel k < Cw.  max_weight is finite and in 1..65504.  A merge is a replace into a scratch volume followed by this
//     per-voxel combine.  Source and destination must not overlap in memory: an overlap is refused.
//
// What follows from it: with R = I, equal resolutions and an origin offset of whole voxels every f_a is 0, only corner 000
// has tw > 0 and the result is a bit copy of the overlap, -0 included (observed voxels only; init_value / 0 elsewhere); a
// 90-degree axis rotation is likewise a permutation; halving the resolution of a fully observed volume is the fp32 mean
// of the 8 children in corner order.  The renormalisation over the counting corners is not linear-exact: only voxels with
// all 8 corners counting reproduce a linear field.
//
// Shape.  Destination-owned: one lane (scalar volumes) or one group of lanes (records) per destination voxel, every output
// written once, no atomics, no LDS, no workspace, the same bits on every run.  A block of 256 lanes owns a tile of
// destination voxels with the lanes running along the contiguous z axis.  Scalar volumes: a wave is one z-run of 64 voxels
// (block 2 x 2 x 64).  Under an axis-aligned M its source voxels are one run as well; under a rotation a compact brick per
// wave (4 x 16, extract's tile of DESIGN 6.7) was measured against it and lost, so the z-run serves every M.
// A lane makes two dependent rounds of loads: the weights of its in-grid corners (which decide what counts, ws, W' and
// the nearest counting corner), then the TSDF of the counting corners together with the id / score of the nearest one -
// and none of the second round for a voxel that is not covered.  When every row of M is a single +-1 and c is whole, g is
// a whole number at every voxel, corner 000 has tw = 1 and the other seven 0: the host launches the same kernels with the
// corner loops cut to that one corner (the same bits by the definition; Database.recentre's case).  Record volumes: a voxel's record is S/8 chunks of 16
// bytes (colour: one chunk of 8 bytes); records of 4 chunks and more get 4 lanes per voxel (lane q takes chunks q, q + 4,
// ... of the 8 corner records; the 8 corner weights are loaded two per lane and passed round the group), smaller records
// one lane; a wave is 16 or 64 voxels of a 4 x 16 tile.  The chunk that holds Cw and padding behind it goes element by
// element, which keeps the padding unread and unwritten; so does everything of a colour volume off the 8-byte grid.
// Record indexing is 64-bit.
#include "ojf_blocks.h"

#include <cmath>

namespace ojf {

constexpr int kResampleBlock = 256;

struct ResampleMap {
    float M[9], c[3];
    int sX, sY, sZ, dX, dY, dZ;
    uint32_t ny, nz;  // tiles along y and z
};

// the destination voxel of slot `slot` of this block's XL x YL x ZL tile; false outside the destination
template <int ZL, int YL, int XL>
__device__ __forceinline__ bool resample_voxel(const ResampleMap &P, int slot, int &i, int &j, int &k)
{
    const uint32_t tile = blockIdx.x;
    const uint32_t tz = tile % P.nz, t = tile / P.nz;
    const uint32_t ty = t % P.ny, tx = t / P.ny;
    k = (int)tz * ZL + (slot % ZL);
    j = (int)ty * YL + ((slot / ZL) % YL);
    i = (int)tx * XL + (slot / (ZL * YL));
    return i < P.dX && j < P.dY && k < P.dZ;
}

// steps 1-3 and the geometric half of step 4: tw[c] and the flat source voxel of every corner that lies in the grid and
// has tw > 0 (-1 for the others).  NC = 1: the host found every g to be a whole number (is_whole_voxel_map), so every f is
// 0 and corner 000, with tw = 1, is the only one with tw > 0 - the other seven are not even formed.
template <int NC>
__device__ __forceinline__ void resample_corners(const ResampleMap &P, int i, int j, int k, float tw[8], int vox[8])
{
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    const int N[3] = {P.sX, P.sY, P.sZ};
    int i0[3];
    float f[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float g = ((P.M[3 * a] * fi + P.M[3 * a + 1] * fj) + P.M[3 * a + 2] * fk) + P.c[a];
        ok = ok && (g >= -1.0f && g <= (float)N[a]);  // (a NaN or inf fails)
        const float fl = floorf(ok ? g : 0.0f);
        f[a] = (ok ? g : 0.0f) - fl;
        i0[a] = (int)fl;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int bi = (c >> 2) & 1, bj = (c >> 1) & 1, bk = c & 1;
        const int ci = i0[0] + bi, cj = i0[1] + bj, ck = i0[2] + bk;
        const float wx = bi ? f[0] : 1.0f - f[0];
        const float wy = bj ? f[1] : 1.0f - f[1];
        const float wz = bk ? f[2] : 1.0f - f[2];
        tw[c] = (wx * wy) * wz;
        const bool in = ok && ci >= 0 && ci < P.sX && cj >= 0 && cj < P.sY && ck >= 0 && ck < P.sZ && tw[c] > 0.0f;
        vox[c] = in ? (ci * P.sY + cj) * P.sZ + ck : -1;
    }
}

// the merge rule of one value: T (or a record channel) and W
__device__ __forceinline__ uint16_t merge_mean(float w0, uint16_t old, float w1, uint16_t fresh)
{
    if (w0 == 0.0f) return fresh;
    return f2h((w0 * h2f(old) + w1 * h2f(fresh)) / (w0 + w1));
}
__device__ __forceinline__ uint16_t merge_weight(float w0, float w1, float max_weight) { return f2h(fminf(w0 + w1, max_weight)); }

// ---- scalar volumes -----------------------------------------------------------------------------------------------------
struct ResampleVolumes {
    ResampleMap map;
    const uint16_t *st, *sw;  // sw null: the ground-truth form
    const uint8_t *si;        // null: no labels
    const uint16_t *ss;
    uint16_t *dt, *dw;
    uint8_t *di;
    uint16_t *ds;
    uint32_t init_bits;
    int merge;
    float max_weight;
};

template <int NC>
__global__ __launch_bounds__(kResampleBlock) void resample_volumes_kernel(ResampleVolumes A)
{
    int i, j, k;
    if (!resample_voxel<64, 2, 2>(A.map, threadIdx.x, i, j, k)) return;
    float tw[8];
    int vox[8];
    resample_corners<NC>(A.map, i, j, k, tw, vox);
    const size_t d = ((size_t)i * A.map.dY + j) * A.map.dZ + k;

    // round 1: the weights of the in-grid corners (and what a merge reads of the destination), all in flight together
    float w[8];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        w[c] = 0.0f;
        if (vox[c] >= 0 && A.sw) w[c] = h2f(A.sw[vox[c]]);
    }
    uint16_t T0 = 0, W0 = 0, S0 = 0;
    if (A.merge) {
        T0 = A.dt[d]; W0 = A.dw[d];
        if (A.di) S0 = A.ds[d];
    }
    // everything but acc follows from the weights: which corners count, ws, W', the nearest counting corner
    float ws = 0.0f, accW = 0.0f, best = 0.0f;
    int bestv = -1;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (vox[c] >= 0 && A.sw && !(w[c] > 0.0f)) vox[c] = -1;  // unobserved
        if (vox[c] < 0) continue;
        ws = ws + tw[c];
        accW = accW + tw[c] * w[c];
        if (tw[c] > best) { best = tw[c]; bestv = vox[c]; }
    }
    bool covered = ws >= 0.5f;
    uint16_t W = 0;
    if (covered && A.sw) {
        W = f2h(accW / ws);
        covered = W != 0;
    }
    if (!covered) {
        if (A.merge) return;
        A.dt[d] = (uint16_t)A.init_bits;
        if (A.dw) A.dw[d] = 0;
        if (A.di) { A.di[d] = 0; A.ds[d] = 0; }
        return;
    }
    // round 2: the values of the counting corners and the label of the nearest one
    float t[8];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        t[c] = 0.0f;
        if (vox[c] >= 0) t[c] = h2f(A.st[vox[c]]);
    }
    uint8_t id = 0;
    uint16_t score = 0;
    if (A.si) { id = A.si[bestv]; score = A.ss[bestv]; }
    float acc = -0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (vox[c] >= 0) acc = acc + tw[c] * t[c];
    const uint16_t T = f2h(acc / ws);
    if (!A.merge) {
        A.dt[d] = T;
        if (A.dw) A.dw[d] = W;
        if (A.di) { A.di[d] = id; A.ds[d] = score; }
        return;
    }
    const float w0 = h2f(W0), w1 = h2f(W);
    A.dt[d] = merge_mean(w0, T0, w1, T);
    A.dw[d] = merge_weight(w0, w1, A.max_weight);
    if (A.di && h2f(score) > h2f(S0)) { A.di[d] = id; A.ds[d] = score; }
}

// ---- record volumes -----------------------------------------------------------------------------------------------------
struct ResampleRecords {
    ResampleMap map;
    const uint16_t *src;
    uint16_t *dst;
    int S, Cw, CH;  // CH: the elements of a chunk, 8 (16 bytes) or 4 (colour: the whole record)
    int vec;        // whole chunks go as one access
    int merge;
    float max_weight;
};

// `n` elements (all CH of them as one access where the volume allows) of a chunk into q
__device__ __forceinline__ void load_chunk(const uint16_t *p, int n, int CH, bool vec, uint32_t q[4])
{
    if (vec && CH == 8) {
        load8(p, 0, q);
    } else if (vec) {
        const uint2 r = *reinterpret_cast<const uint2 *>(p);
        q[0] = r.x; q[1] = r.y; q[2] = 0; q[3] = 0;
    } else {
        q[0] = q[1] = q[2] = q[3] = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < n) set16(q, e, p[e]);
    }
}

template <int G, int NC>
__global__ __launch_bounds__(kResampleBlock) void resample_records_kernel(ResampleRecords A)
{
    constexpr int ZL = 16, YL = 4, XL = kResampleBlock / G / (ZL * YL);
    const int sub = threadIdx.x % G;
    int i, j, k;
    if (!resample_voxel<ZL, YL, XL>(A.map, threadIdx.x / G, i, j, k)) return;  // (a whole group leaves together)
    float tw[8];
    int vox[8];
    resample_corners<NC>(A.map, i, j, k, tw, vox);
    const size_t S = (size_t)A.S;

    float w[8];
#pragma unroll
    for (int c = 0; c < NC; ++c) {  // lane q of a group loads the weights of corners q and q + 4 for all of it
        float mine = 0.0f;
        if (vox[c] >= 0 && (c % G) == sub) mine = h2f(A.src[(size_t)vox[c] * S + A.Cw]);
        w[c] = G == 1 ? mine : __shfl(mine, c % G, G);
    }
    float ws = 0.0f, accW = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (!(w[c] > 0.0f)) { vox[c] = -1; continue; }
        ws = ws + tw[c];
        accW = accW + tw[c] * w[c];
    }
    bool covered = ws >= 0.5f;
    uint16_t W = 0;
    if (covered) {
        W = f2h(accW / ws);
        covered = W != 0;
    }
    if (!covered && A.merge) return;
    uint16_t *const drec = A.dst + (((size_t)i * A.map.dY + j) * A.map.dZ + k) * S;
    float w0 = 0.0f;
    const float w1 = h2f(W);
    if (A.merge) w0 = h2f(drec[A.Cw]);  // (read by every lane of the group before the lane that owns the chunk stores it)

    const int chunks = A.Cw / A.CH + 1;  // the chunks that hold channels 0..Cw
    for (int ch = sub; ch < chunks; ch += G) {
        const int base = ch * A.CH;
        const int n = A.Cw + 1 - base < A.CH ? A.Cw + 1 - base : A.CH;
        const bool vec = A.vec && n == A.CH;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = -0.0f;
        if (covered) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (vox[c] < 0) continue;
                uint32_t q[4];
                load_chunk(A.src + (size_t)vox[c] * S + base, n, A.CH, vec, q);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = acc[e] + tw[c] * h2f((uint16_t)get16(q, e));
            }
        }
        uint32_t old[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0};
        if (A.merge) load_chunk(drec + base, n, A.CH, vec, old);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e >= n) continue;
            uint16_t v = 0;
            if (covered) {
                const bool is_w = base + e == A.Cw;
                v = is_w ? W : f2h(acc[e] / ws);
                if (A.merge) v = is_w ? merge_weight(w0, w1, A.max_weight) : merge_mean(w0, (uint16_t)get16(old, e), w1, v);
            }
            set16(out, e, v);
        }
        if (vec && A.CH == 8) {
            *reinterpret_cast<uint4 *>(drec + base) = make_uint4(out[0], out[1], out[2], out[3]);
        } else if (vec) {
            *reinterpret_cast<uint2 *>(drec + base) = make_uint2(out[0], out[1]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < n) drec[base + e] = (uint16_t)get16(out, e);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

// everything the two entry points check alike; fills the map (tile counts excepted)
static int check_resample(const char *who, int sX, int sY, int sZ, int dX, int dY, int dZ, const double *M, const double *c, int mode,
                          float max_weight, ResampleMap &P)
{
    if (!M || !c) return refuse(who, "null pointer argument");
    if (int rc = check_volume_size(who, sX, sY, sZ)) return rc;
    if (int rc = check_volume_size(who, dX, dY, dZ)) return rc;
    if (mode != OJF_RESAMPLE_REPLACE && mode != OJF_RESAMPLE_MERGE) return refuse(who, "unknown mode");
    if (!all_finite(M, 9) || !all_finite(c, 3)) return refuse(who, "non-finite M or c");
    for (int i = 0; i < 9; ++i) P.M[i] = (float)M[i];
    for (int i = 0; i < 3; ++i) P.c[i] = (float)c[i];
    bool finite = true;
    for (int i = 0; i < 9; ++i) finite &= std::isfinite(P.M[i]);
    for (int i = 0; i < 3; ++i) finite &= std::isfinite(P.c[i]);
    if (!finite) return refuse(who, "non-finite M or c in fp32");
    if (!(max_weight >= 1.0f && max_weight <= 65504.0f)) return refuse(who, "max_weight must be in 1..65504");
    P.sX = sX; P.sY = sY; P.sZ = sZ; P.dX = dX; P.dY = dY; P.dZ = dZ;
    return 0;
}

// every row of M is a single +-1 and c is whole (as fp32): g is a whole number at every destination voxel - whole-voxel
// shifts, axis flips and permutations (Database.recentre's case)
static bool is_whole_voxel_map(const ResampleMap &P)
{
    const int lim = 1 << 22;  // indices and |c| up to 2^22: |g| <= 2^23, every product and sum of step 1 is exact
    if (P.dX > lim || P.dY > lim || P.dZ > lim) return false;
    for (int a = 0; a < 3; ++a) {
        int ones = 0;
        for (int b = 0; b < 3; ++b) {
            const float m = P.M[3 * a + b];
            if (m == 1.0f || m == -1.0f) ++ones;
            else if (m != 0.0f) return false;
        }
        if (ones != 1 || P.c[a] != std::floor(P.c[a]) || std::fabs(P.c[a]) > (float)lim) return false;
    }
    return true;
}

static int resample_tiles(const char *who, ResampleMap &P, int XL, int YL, int ZL, uint32_t &blocks)
{
    const int64_t nx = (P.dX + XL - 1) / XL, ny = (P.dY + YL - 1) / YL, nz = (P.dZ + ZL - 1) / ZL;
    if (!volume_size_ok(nx, ny, nz)) return refuse(who, "volume too large");
    P.ny = (uint32_t)ny; P.nz = (uint32_t)nz;
    blocks = (uint32_t)(nx * ny * nz);
    return 0;
}

}  // namespace ojf

OJF_API int ojf_resample_volumes(const uint16_t *src_tsdf, const uint16_t *src_weights, const uint8_t *src_ids, const uint16_t *src_scores,
                                 int sX, int sY, int sZ, uint16_t *dst_tsdf, uint16_t *dst_weights, uint8_t *dst_ids, uint16_t *dst_scores,
                                 int dX, int dY, int dZ, const double *M, const double *c, float init_value, int mode, float max_weight,
                                 ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_resample_volumes";
    if (!src_tsdf || !dst_tsdf) return refuse(who, "null pointer argument");
    if ((src_weights != nullptr) != (dst_weights != nullptr)) return refuse(who, "weights must be given on both sides or on neither");
    const int n_label = (src_ids != nullptr) + (src_scores != nullptr) + (dst_ids != nullptr) + (dst_scores != nullptr);
    if (n_label != 0 && n_label != 4) return refuse(who, "ids and scores must be all set or all NULL");
    ResampleVolumes A;
    if (int rc = check_resample(who, sX, sY, sZ, dX, dY, dZ, M, c, mode, max_weight, A.map)) return rc;
    if (!std::isfinite(init_value)) return refuse(who, "non-finite init_value");
    if (mode == OJF_RESAMPLE_MERGE && !src_weights) return refuse(who, "merge mode needs the weight volumes");
    if (((uintptr_t)src_tsdf | (uintptr_t)src_weights | (uintptr_t)src_scores | (uintptr_t)dst_tsdf | (uintptr_t)dst_weights |
         (uintptr_t)dst_scores) & 1)
        return refuse(who, "fp16 volumes must be 2-byte aligned");
    const size_t ns = (size_t)sX * sY * sZ, nd = (size_t)dX * dY * dZ;
    const void *srcs[4] = {src_tsdf, src_weights, src_ids, src_scores};
    const void *dsts[4] = {dst_tsdf, dst_weights, dst_ids, dst_scores};
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b)
            if (ranges_overlap(srcs[a], ns * (a == 2 ? 1 : 2), dsts[b], nd * (b == 2 ? 1 : 2)))
                return refuse(who, "source and destination volumes overlap");
    A.st = src_tsdf; A.sw = src_weights; A.si = src_ids; A.ss = src_scores;
    A.dt = dst_tsdf; A.dw = dst_weights; A.di = dst_ids; A.ds = dst_scores;
    A.init_bits = __builtin_bit_cast(uint16_t, (_Float16)init_value);
    A.merge = mode == OJF_RESAMPLE_MERGE;
    A.max_weight = max_weight;
    uint32_t blocks;
    if (int rc = resample_tiles(who, A.map, 2, 2, 64, blocks)) return rc;
    if (is_whole_voxel_map(A.map)) hipLaunchKernelGGL(resample_volumes_kernel<1>, dim3(blocks), dim3(kResampleBlock), 0, as_stream(stream), A);
    else hipLaunchKernelGGL(resample_volumes_kernel<8>, dim3(blocks), dim3(kResampleBlock), 0, as_stream(stream), A);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_resample_records(const uint16_t *src, int sX, int sY, int sZ, uint16_t *dst, int dX, int dY, int dZ, int S, int Cw,
                                 const double *M, const double *c, int mode, float max_weight, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_resample_records";
    if (!src || !dst) return refuse(who, "null pointer argument");
    ResampleRecords A;
    if (int rc = check_resample(who, sX, sY, sZ, dX, dY, dZ, M, c, mode, max_weight, A.map)) return rc;
    if (!(S == 4 || (S > 0 && S % 8 == 0)) || S > 264) return refuse(who, "S must be 4 (colour) or a multiple of 8 up to 264");
    if (Cw <= 0 || Cw >= S) return refuse(who, "Cw must be in 1..S-1");
    if (S == 4 ? (((uintptr_t)src | (uintptr_t)dst) & 1) != 0 : (((uintptr_t)src | (uintptr_t)dst) & 15) != 0)
        return refuse(who, "records must be 16-byte aligned (colour records: 2-byte)");
    if (ranges_overlap(src, (size_t)sX * sY * sZ * S * 2, dst, (size_t)dX * dY * dZ * S * 2))
        return refuse(who, "source and destination volumes overlap");
    A.src = src; A.dst = dst;
    A.S = S; A.Cw = Cw; A.CH = S == 4 ? 4 : 8;
    A.vec = S == 4 ? (((uintptr_t)src | (uintptr_t)dst) & 7) == 0 : 1;  // a colour volume off the 8-byte grid goes element by element
    A.merge = mode == OJF_RESAMPLE_MERGE;
    A.max_weight = max_weight;
    const bool whole = is_whole_voxel_map(A.map);
    uint32_t blocks;
    if (Cw / A.CH + 1 >= 4) {
        if (int rc = resample_tiles(who, A.map, 1, 4, 16, blocks)) return rc;
        if (whole) hipLaunchKernelGGL((resample_records_kernel<4, 1>), dim3(blocks), dim3(kResampleBlock), 0, as_stream(stream), A);
        else hipLaunchKernelGGL((resample_records_kernel<4, 8>), dim3(blocks), dim3(kResampleBlock), 0, as_stream(stream), A);
    } else {
        if (int rc = resample_tiles(who, A.map, 4, 4, 16, blocks)) return rc;
        if (whole) hipLaunchKernelGGL((resample_records_kernel<1, 1>), dim3(blocks), dim3(kResampleBlock), 0, as_stream(stream), A);
        else hipLaunchKernelGGL((resample_records_kernel<1, 8>), dim3(blocks), dim3(kResampleBlock), 0, as_stream(stream), A);
    }
    OJF_HIP(hipGetLastError());
    return 0;
}
