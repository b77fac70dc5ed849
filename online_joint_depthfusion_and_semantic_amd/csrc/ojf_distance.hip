// EXACT EUCLIDEAN DISTANCE TRANSFORM of a volume, with the nearest seed of every voxel (the feature transform), and what is
// built on it: the surface voxels of a fused TSDF and its ESDF.  Metric dilation and erosion of masks and "the label of the
// nearest labelled voxel" (distance.py) come from the same two arrays.  tests/distance_ref.py restates the definition in
// numpy and the GPU tests pin the kernels to it bit for bit.
//
// Normative definition.  Volumes are [X,Y,Z] with z contiguous; the linear index of a voxel is v = (x·Y + y)·Z + z.
//   1 <= X, Y, Z <= 2048 and X·Y·Z < 2^31, so d² <= 3·2047² < 2^24.
//   seeds u8: a voxel is a seed where the byte is non-zero.
//   dist2 i32 [X,Y,Z]: the minimum over the seeds q of |p - q|², in voxel units.
//   nearest i32 [X,Y,Z]: the smallest linear index among the seeds that attain that minimum.  The pair is the minimum of the
//     64-bit key (d² << 32) | index(q): a property of the input alone, the same bits on every run and for every algorithm.
//   With no seed in reach dist2 = 2^31 - 1 (OJF_EDT_NONE) and nearest = -1.
//   max_dist2, an integer, negative = unlimited: a voxel with d² > max_dist2 gets NONE / -1, every other voxel is unchanged
//     from the unlimited result.
//   Separable form: a 1-D pass along z, then y, then x, g'[c] = min over c' of g[c'] + (c - c')², each pass breaking ties
//     towards the smaller source coordinate c'.  This yields exactly the smallest-linear-index rule (checked on the host
//     against brute-force keys, tests/test_distance_host.py).  A partial sum never exceeds the final one, so every pass may
//     write NONE / -1 where its result exceeds max_dist2 and look no further than floor(sqrt(max_dist2)) along its axis.
// Surface mask (ojf_volume_surface_mask): 1 where a voxel is observed by ojf_volume_observed_mask's rule without a band
//   (fp32(weight) > 0 and a TSDF value that is no NaN) and has an observed face neighbour on the other side of the surface;
//   "inside" is fp32(tsdf) < 0, so -0.0 and +0.0 are outside.  Else 0.
// ESDF (ojf_volume_esdf): esdf[p] = s · (fp32(resolution) · sqrtf((float)dist2[p])) - one correctly rounded square root and
//   one correctly rounded product (the Makefile's flags) -, s = -1 where p is observed and inside, else +1 (an unobserved
//   voxel gets the unsigned distance).  Where dist2 is NONE, esdf[p] = s · far.  The accuracy is that of voxel centres.
//
// Tile.  Two extents, both along z:
//   the z pass works in CHUNKS of 64 voxels (kDChunk, one per lane of a wave);
//   the y and x passes own whole lines along their axis for a RUN of R consecutive z, R = min(64, 20480 / L, Z) for lines of
//     L voxels (kDMaxRun, kDLdsInts): 4 B per staged voxel, at most 80 KiB of the CU's 160 KiB of LDS per block, so that two
//     blocks share a CU.  R = 64 up to L = 320, 63 at L = 321, 10 at L = 2048.
// Passes (kernel boundaries separate them; no thread waits for another workgroup):
//   z  (edt_z_kernel): a wave owns a z line.  It reads the seeds chunk by chunk; lane j keeps the ballot of chunk j (a line
//     has at most 32 chunks).  Count-leading / trailing-zeros of a lane's own chunk mask below and above its bit give the
//     nearest seed in the chunk; where the chunk has none on that side, the last seed of the nearest non-empty chunk before
//     and the first of the nearest one behind it (a ballot of "my chunk has a seed", again clz / ctz, one shuffle) are the
//     carry.  Of two seeds at equal distance the one below wins.  Out: d² and the seed's linear index.
//   y, x (edt_line_kernel): a block of 1024 lanes owns the lines along the pass axis of one outer index (x for the y pass, y
//     for the x pass) and one run of z; global accesses are R consecutive voxels wide.  It stages the lines' d² in LDS as
//     g[c·R + r], and every (c, r) walks outwards from c: k = 1, 2, ... while k² <= the best found, k² <= max_dist2 and a
//     side is left, taking c - k when it is no worse (ties go down) and c + k when it is better.  Exact, and short near
//     the surface.  The index follows by a gather from the winner's voxel after the search.  d² is rewritten in place (the
//     block owns its lines and has staged them); the index goes from one array to another - the z pass writes nearest, the
//     y pass nearest -> workspace, the x pass workspace -> nearest - since a gather may read a voxel another lane rewrites.
//   finish (surface_mask_kernel, esdf_kernel): streaming, one lane per 8 consecutive voxels with 16-byte loads of the fp16
//     volumes where the pointers (and for the mask, the z rows) allow it, one voxel per lane otherwise.
#include "ojf_blocks.h"

namespace ojf {

constexpr int kDBlock = 256;      // lanes per block of the z pass and the finishing kernels
constexpr int kDLineBlock = 1024;  // y / x pass: lanes per block - two blocks of 80 KiB fill a CU's 32 wave slots
constexpr int kDChunk = 64;       // z pass: voxels per ballot
constexpr int kDMaxRun = 64;      // y / x pass: the longest run of z a block owns
constexpr int kDLdsInts = 20480;  // y / x pass: staged voxels per block (80 KiB)
constexpr int kDMaxDim = 2048;
constexpr uint32_t kDNone = (uint32_t)OJF_EDT_NONE;

// ---- z ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(kDBlock) void edt_z_kernel(const uint8_t *seeds, uint32_t lines, int Z, uint32_t lim, int *dist2, int *nearest)
{
    const int lane = threadIdx.x & 63;
    const uint32_t line = blockIdx.x * (uint32_t)(kDBlock / 64) + (threadIdx.x >> 6);
    if (line >= lines) return;  // (the whole wave)
    const size_t base = (size_t)line * (size_t)Z;
    const int chunks = (Z + kDChunk - 1) / kDChunk;  // <= 32
    unsigned long long mine = 0ull;                  // lane j: the seeds of chunk j
    for (int j = 0; j < chunks; ++j) {
        const int z = j * kDChunk + lane;
        const unsigned long long m = __ballot(z < Z && seeds[base + z] != 0);
        if (lane == j) mine = m;
    }
    const int first = mine ? lane * kDChunk + __builtin_ctzll(mine) : -1;
    const int last = mine ? lane * kDChunk + 63 - __builtin_clzll(mine) : -1;
    const unsigned long long occupied = __ballot(mine != 0ull);
    for (int j = 0; j < chunks; ++j) {
        const unsigned long long own = shfl64(mine, j);
        const unsigned long long before = occupied & ((1ull << j) - 1ull), behind = occupied & ~((2ull << j) - 1ull);
        const int from_before = __shfl(last, before ? 63 - __builtin_clzll(before) : 0);
        const int from_behind = __shfl(first, behind ? __builtin_ctzll(behind) : 0);
        const int z = j * kDChunk + lane;
        if (z >= Z) continue;  // (every shuffle of this round is behind us)
        const unsigned long long lo = own & ((2ull << lane) - 1ull), hi = own & ~((1ull << lane) - 1ull);
        const int zb = lo ? j * kDChunk + 63 - __builtin_clzll(lo) : (before ? from_before : -1);
        const int za = hi ? j * kDChunk + __builtin_ctzll(hi) : (behind ? from_behind : -1);
        uint32_t d2 = kDNone;
        int idx = -1;
        if (zb >= 0 || za >= 0) {
            const int db = zb >= 0 ? z - zb : kDMaxDim, da = za >= 0 ? za - z : kDMaxDim;
            const int d = db <= da ? db : da;  // a tie goes to the seed below
            if ((uint32_t)(d * d) <= lim) {
                d2 = (uint32_t)(d * d);
                idx = (int)(base + (size_t)(db <= da ? zb : za));
            }
        }
        dist2[base + z] = (int)d2;
        nearest[base + z] = idx;
    }
}

// ---- y, x ------------------------------------------------------------------------------------------------------------
struct LineArgs {
    int L, Z, R, runs;              // line length, z extent, z run, runs per z row
    uint32_t stride, outer_stride;  // between neighbours of a line / between the outer indices, in voxels
    uint32_t lim;                   // the largest d² that is kept
    int klim;                       // min(L - 1, floor(sqrt(lim)))
    int *dist2;                     // in place
    const int *near_in;
    int *near_out;
};

__global__ __launch_bounds__(kDLineBlock) void edt_line_kernel(LineArgs a)
{
    extern __shared__ uint32_t edt_g[];  // [L][rn]
    const uint32_t outer = blockIdx.x / (uint32_t)a.runs, run = blockIdx.x % (uint32_t)a.runs;
    const int z0 = (int)run * a.R;
    const int rn = min(a.R, a.Z - z0);  // >= 1: runs = ceil(Z / R)
    const size_t base = (size_t)outer * a.outer_stride + (size_t)z0;
    const int n = a.L * rn;  // <= kDLdsInts
    for (int i = threadIdx.x; i < n; i += kDLineBlock) {
        const int c = i / rn, r = i - c * rn;
        edt_g[i] = (uint32_t)a.dist2[base + (size_t)c * a.stride + r];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kDLineBlock) {
        const int c = i / rn, r = i - c * rn;
        uint32_t best = edt_g[i];
        int bc = c;
        const int kmax = min(a.klim, max(c, a.L - 1 - c));
        for (int k = 1; k <= kmax; ++k) {
            const uint32_t kk = (uint32_t)(k * k);
            if (kk > best) break;  // (kk == best can still tie, from a seed line, and a tie below wins)
            if (c - k >= 0) {
                const uint32_t v = edt_g[i - k * rn] + kk;  // NONE + k² < 2^32
                if (v <= best) { best = v; bc = c - k; }
            }
            if (c + k < a.L) {
                const uint32_t v = edt_g[i + k * rn] + kk;
                if (v < best) { best = v; bc = c + k; }
            }
        }
        const size_t at = base + (size_t)c * a.stride + r;
        if (best <= a.lim) {
            a.dist2[at] = (int)best;
            a.near_out[at] = a.near_in[base + (size_t)bc * a.stride + r];
        } else {
            a.dist2[at] = (int)kDNone;
            a.near_out[at] = -1;
        }
    }
}

// ---- surface mask, ESDF --------------------------------------------------------------------------------------------------
// 0: unobserved, 1: observed and outside, 2: observed and inside; two voxels face each other across the surface when the
// exclusive or of their states is 3
__device__ __forceinline__ uint32_t surf_state(uint16_t t, uint16_t w) { return voxel_observed(t, w) ? (h2f(t) < 0.0f ? 2u : 1u) : 0u; }

__global__ __launch_bounds__(kDBlock) void surface_mask_kernel(const uint16_t *tsdf, const uint16_t *wgt, int X, int Y, int Z, uint8_t *mask)
{
    const size_t n = (size_t)X * Y * Z;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t sy = (size_t)Z, sx = (size_t)Y * Z;
    // 8 voxels of one z row per lane: every row starts on a 16-byte boundary
    if ((Z & 7) == 0 && (((uintptr_t)tsdf | (uintptr_t)wgt) & 15) == 0 && ((uintptr_t)mask & 7) == 0) {
        const int zg = Z >> 3;
        for (size_t g = tid; g < n / 8; g += step) {
            const int z0 = (int)(g % (size_t)zg) * 8;
            const int y = (int)((g / (size_t)zg) % (size_t)Y), x = (int)(g / ((size_t)zg * Y));
            const size_t v0 = g * 8;
            uint32_t tq[4], wq[4], s[10], hit[8];
            load8(tsdf, g, tq);
            load8(wgt, g, wq);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s[e + 1] = surf_state((uint16_t)get16(tq, e), (uint16_t)get16(wq, e));
                hit[e] = 0u;
            }
            s[0] = z0 > 0 ? surf_state(tsdf[v0 - 1], wgt[v0 - 1]) : 0u;
            s[9] = z0 + 8 < Z ? surf_state(tsdf[v0 + 8], wgt[v0 + 8]) : 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) hit[e] |= (uint32_t)((s[e + 1] ^ s[e]) == 3u) | (uint32_t)((s[e + 1] ^ s[e + 2]) == 3u);
#pragma unroll
            for (int side = 0; side < 4; ++side) {
                const bool in = side == 0 ? y > 0 : side == 1 ? y + 1 < Y : side == 2 ? x > 0 : x + 1 < X;
                if (!in) continue;
                const size_t u = side == 0 ? v0 - sy : side == 1 ? v0 + sy : side == 2 ? v0 - sx : v0 + sx;
                load8(tsdf, u / 8, tq);
                load8(wgt, u / 8, wq);
#pragma unroll
                for (int e = 0; e < 8; ++e) hit[e] |= (uint32_t)((s[e + 1] ^ surf_state((uint16_t)get16(tq, e), (uint16_t)get16(wq, e))) == 3u);
            }
            uint32_t out[2] = {0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; ++e) out[e >> 2] |= hit[e] << (8 * (e & 3));
            reinterpret_cast<uint2 *>(mask)[g] = make_uint2(out[0], out[1]);
        }
        return;
    }
    for (size_t v = tid; v < n; v += step) {
        const int z = (int)(v % (size_t)Z), y = (int)((v / (size_t)Z) % (size_t)Y), x = (int)(v / sx);
        const uint32_t s = surf_state(tsdf[v], wgt[v]);
        uint32_t hit = 0u;
        if (s) {
            if (z > 0) hit |= (uint32_t)((s ^ surf_state(tsdf[v - 1], wgt[v - 1])) == 3u);
            if (z + 1 < Z) hit |= (uint32_t)((s ^ surf_state(tsdf[v + 1], wgt[v + 1])) == 3u);
            if (y > 0) hit |= (uint32_t)((s ^ surf_state(tsdf[v - sy], wgt[v - sy])) == 3u);
            if (y + 1 < Y) hit |= (uint32_t)((s ^ surf_state(tsdf[v + sy], wgt[v + sy])) == 3u);
            if (x > 0) hit |= (uint32_t)((s ^ surf_state(tsdf[v - sx], wgt[v - sx])) == 3u);
            if (x + 1 < X) hit |= (uint32_t)((s ^ surf_state(tsdf[v + sx], wgt[v + sx])) == 3u);
        }
        mask[v] = (uint8_t)hit;
    }
}

__device__ __forceinline__ float esdf_value(int d2, uint16_t t, uint16_t w, float res, float far)
{
    const float mag = (uint32_t)d2 == kDNone ? far : res * sqrtf((float)d2);
    return surf_state(t, w) == 2u ? -mag : mag;
}

__global__ __launch_bounds__(kDBlock) void esdf_kernel(const int *dist2, const uint16_t *tsdf, const uint16_t *wgt, size_t n, float res, float far,
                                                       float *esdf)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const bool aligned = (((uintptr_t)tsdf | (uintptr_t)wgt | (uintptr_t)dist2 | (uintptr_t)esdf) & 15) == 0;
    const size_t nvec = aligned ? n / 8 : 0;
    for (size_t i = tid; i < nvec; i += step) {
        uint32_t tq[4], wq[4];
        load8(tsdf, i, tq);
        load8(wgt, i, wq);
        const int4 da = reinterpret_cast<const int4 *>(dist2)[2 * i], db = reinterpret_cast<const int4 *>(dist2)[2 * i + 1];
        const int d[8] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = esdf_value(d[e], (uint16_t)get16(tq, e), (uint16_t)get16(wq, e), res, far);
        reinterpret_cast<float4 *>(esdf)[2 * i] = make_float4(o[0], o[1], o[2], o[3]);
        reinterpret_cast<float4 *>(esdf)[2 * i + 1] = make_float4(o[4], o[5], o[6], o[7]);
    }
    for (size_t i = nvec * 8 + tid; i < n; i += step) esdf[i] = esdf_value(dist2[i], tsdf[i], wgt[i], res, far);
}

static inline bool edt_dims_ok(int X, int Y, int Z) { return X >= 1 && Y >= 1 && Z >= 1 && X <= kDMaxDim && Y <= kDMaxDim && Z <= kDMaxDim; }

static inline int check_edt_size(const char *who, int X, int Y, int Z)
{
    if (!edt_dims_ok(X, Y, Z)) return refuse(who, "X, Y and Z must be in 1..2048");
    return check_volume_size(who, X, Y, Z);
}

static int launch_line_pass(int L, int outer, uint32_t stride, uint32_t outer_stride, int Z, uint32_t lim, int *dist2, const int *near_in,
                            int *near_out, hipStream_t s)
{
    static bool configured = false;
    if (!configured) {
        OJF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&edt_line_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kDLdsInts * sizeof(uint32_t))));
        configured = true;
    }
    LineArgs a;
    a.L = L; a.Z = Z;
    a.R = kDLdsInts / L < kDMaxRun ? kDLdsInts / L : kDMaxRun;
    if (a.R > Z) a.R = Z;
    a.runs = (Z + a.R - 1) / a.R;
    a.stride = stride; a.outer_stride = outer_stride;
    a.lim = lim;
    int k = 0;
    while (k < L - 1 && (uint64_t)(k + 1) * (uint64_t)(k + 1) <= lim) ++k;
    a.klim = k;
    a.dist2 = dist2; a.near_in = near_in; a.near_out = near_out;
    hipLaunchKernelGGL(edt_line_kernel, dim3((uint32_t)outer * (uint32_t)a.runs), dim3(kDLineBlock), (size_t)L * a.R * sizeof(uint32_t), s, a);
    OJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace ojf

OJF_API size_t ojf_volume_edt_workspace_bytes(int X, int Y, int Z)
{
    if (!ojf::edt_dims_ok(X, Y, Z) || !ojf::volume_size_ok(X, Y, Z)) return 0;
    return ((size_t)X * Y * Z * sizeof(int32_t) + 7) & ~(size_t)7;  // the index array the y pass writes and the x pass reads
}

OJF_API int ojf_volume_edt(const uint8_t *seeds, int X, int Y, int Z, int max_dist2, int phases, void *workspace, size_t workspace_bytes,
                           int32_t *dist2, int32_t *nearest, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_volume_edt";
    if (!seeds || !workspace || !dist2 || !nearest) return refuse(who, "null pointer argument");
    if (int rc = check_edt_size(who, X, Y, Z)) return rc;
    if (phases < 1 || phases > OJF_EDT_ALL) return refuse(who, "phases must be a non-empty set of OJF_EDT_* bits");
    if (workspace_bytes < ojf_volume_edt_workspace_bytes(X, Y, Z)) return refuse(who, "workspace too small");
    if (((uintptr_t)workspace & 7) || ((uintptr_t)dist2 & 3) || ((uintptr_t)nearest & 3))
        return refuse(who, "workspace_dev must be 8-byte, the i32 arrays 4-byte aligned");

    const uint32_t lim = max_dist2 < 0 ? kDNone - 1u : (uint32_t)max_dist2;  // (NONE itself is never kept)
    int *const side = reinterpret_cast<int *>(workspace);
    hipStream_t s = as_stream(stream);
    if (phases & OJF_EDT_Z) {
        const uint32_t lines = (uint32_t)X * (uint32_t)Y;
        hipLaunchKernelGGL(edt_z_kernel, dim3((lines + kDBlock / 64 - 1) / (kDBlock / 64)), dim3(kDBlock), 0, s, seeds, lines, Z, lim, dist2, nearest);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_EDT_Y)
        if (int rc = launch_line_pass(Y, X, (uint32_t)Z, (uint32_t)Y * (uint32_t)Z, Z, lim, dist2, nearest, side, s)) return rc;
    if (phases & OJF_EDT_X)
        if (int rc = launch_line_pass(X, Y, (uint32_t)Y * (uint32_t)Z, (uint32_t)Z, Z, lim, dist2, side, nearest, s)) return rc;
    return 0;
}

OJF_API int ojf_volume_surface_mask(const uint16_t *tsdf, const uint16_t *wgt, int X, int Y, int Z, uint8_t *mask, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_volume_surface_mask";
    if (!tsdf || !wgt || !mask) return refuse(who, "null pointer argument");
    if (int rc = check_edt_size(who, X, Y, Z)) return rc;
    if (((uintptr_t)tsdf & 1) || ((uintptr_t)wgt & 1)) return refuse(who, "tsdf_dev and weights_dev must be 2-byte aligned");
    const size_t n = (size_t)X * Y * Z;
    hipLaunchKernelGGL(surface_mask_kernel, dim3(stream_grid((Z & 7) ? n : n / 8, kDBlock)), dim3(kDBlock), 0, as_stream(stream), tsdf, wgt, X, Y, Z,
                       mask);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_volume_esdf(const int32_t *dist2, const uint16_t *tsdf, const uint16_t *wgt, size_t n, float resolution, float far, float *esdf,
                            ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_volume_esdf";
    if (!dist2 || !tsdf || !wgt || !esdf) return refuse(who, "null pointer argument");
    if (n == 0 || n > 0x7fffffffULL) return refuse(who, "the voxel count must be in 1..2^31-1");
    if (!(resolution > 0.0f) || !(resolution < INFINITY)) return refuse(who, "resolution must be > 0 and finite");
    if (!(far >= 0.0f)) return refuse(who, "far must be >= 0 (a NaN is refused)");
    if (((uintptr_t)dist2 & 3) || ((uintptr_t)esdf & 3) || ((uintptr_t)tsdf & 1) || ((uintptr_t)wgt & 1))
        return refuse(who, "dist2_dev and esdf_dev must be 4-byte, the volumes 2-byte aligned");
    hipLaunchKernelGGL(esdf_kernel, dim3(stream_grid(n / 8 + 1, kDBlock)), dim3(kDBlock), 0, as_stream(stream), dist2, tsdf, wgt, n, resolution, far,
                       esdf);
    OJF_HIP(hipGetLastError());
    return 0;
}
