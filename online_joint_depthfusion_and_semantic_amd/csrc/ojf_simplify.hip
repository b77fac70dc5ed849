// SIMPLIFY: vertex clustering of an indexed triangle mesh with quadric error metrics (Lindstrom's out-of-core simplification;
// the third stage of the reference's deps/mesh-fusion, which shells out to meshlabserver on the host).  Own design: a uniform
// grid of cells cuts the mesh, all vertices of a cell become ONE vertex placed where the summed plane quadric of the incident
// faces is smallest, faces that lose a corner disappear.  The definition - every rounding point - is in DESIGN.md §19 and
// restated in numpy by tests/simplify_ref.py; the kernels are held to it bit for bit.
//
// Every step is a map, a scan or an INTEGER atomic, so the result is a function of the input alone (the one exception, by
// definition: `source` at exact ties goes to the lower vertex index - which is what the 64-bit minimum gives).  Phases, each a
// kernel boundary, no thread waits for another workgroup:
//   MARK        per vertex: cell index and local position (1/256 cell around the cell centre, packed 3 x 9 bits), and the
//               cell's bit in a bitmap (atomicOr; one BIT per cell: 256^3 cells are 2 MB).
//   SCAN        exclusive prefix of the per-word popcounts (one workgroup: ojf_blocks.h's block_exclusive_scan), counts[0] = the
//               number of occupied cells = output vertices; then per vertex cluster = prefix[word] + popcount(bits below).
//   COUNT       per block of 256 faces the number of kept faces, the same scan over the blocks, counts[1] = kept faces.
//   ACCUMULATE  128-byte accumulator row per cluster, zeroed; per occupied cell its index into the row; per vertex S += p,
//               cnt += 1; per face and corner A += w n n^T, b += w d n - 64-bit integer atomicAdd, exact, so the order in
//               which they land cannot show.  Consecutive vertices and faces of an extracted mesh share cells, so every run
//               of lanes of a wave with the same cluster is summed in registers first and its last lane issues the atomics:
//               measured against one atomic per lane this takes the phase from 3.3 to 0.95 ms on the 2 M
//               faces of the 256^3 room at 2 voxels per cell.
//   SOLVE       per cluster the 3x3 solve in f64 with a Tikhonov term towards the vertex mean; the position.
//   NEAREST     per vertex a 64-bit atomicMin of (bits(d^2) << 32) | vertex on its cluster's row, then per cluster `source`.
//   FACES       per block of faces: the kept ones, renamed to clusters, at the block's offset in input order (no atomics).
// Between COUNT and the rest the host reads the two counts to size the outputs and the rows (the protocol of ojf_mesh_extract).
//
// Overflow: |p| <= 2^7, |n| <= 2^9, 1 <= w <= 2^10, so |d| = |n.p| <= 3 2^16, one term of b is at most
// 2^10 3 2^16 2^9 = 3 2^35 and one of A at most 2^10 2^18 = 2^28.  A face is added once per corner: at most 3 2^24 incidences
// in all, hence |b| <= 9 2^59 < 2^63 and |A| <= 3 2^52; |S| <= 2^7 nv < 2^38.  The static_asserts below repeat this.
#include "ojf_blocks.h"

#include <math.h>

namespace ojf {

constexpr int kSBlock = 256;            // threads per block, and faces per block of the count / fill pair
constexpr int64_t kSMaxFaces = 1 << 24;
constexpr int kSPosMax = 128, kSNormalMax = 512, kSWeightMax = 1024;
constexpr int64_t kSIncidences = 3 * kSMaxFaces;
static_assert((int64_t)kSWeightMax * (3 * kSNormalMax * kSPosMax) * kSNormalMax == (3LL << 35), "one term of b");
static_assert((3LL << 35) <= INT64_MAX / kSIncidences, "b stays below 2^63 over 3 * 2^24 incidences");
static_assert((int64_t)kSWeightMax * kSNormalMax * kSNormalMax <= INT64_MAX / kSIncidences / 3, "A, and the trace of A, stay below 2^63");
static_assert((int64_t)kSPosMax * INT32_MAX < INT64_MAX, "S stays below 2^63");

struct SimplifyRow {
    long long A[6];   // 00 01 02 11 12 22
    long long b[3];
    long long S[3];
    long long cnt;
    int cell;         // written per occupied cell before the sums
    float rep[3];     // SOLVE: the representative, for NEAREST (the output may be cut short by its capacity)
    unsigned long long key;  // SOLVE: ~0; NEAREST: the minimum
};
static_assert(sizeof(SimplifyRow) == 128, "one accumulator row is 128 bytes");

struct SimplifyArgs {
    const float *verts;
    const int *faces;
    int nv, nf;
    float lo[3], cell;
    int G[3];
    uint32_t words;       // bitmap words
    uint32_t fblocks_n;   // blocks of faces
    int *vcell;           // [nv] cell index, -1: invalid
    uint32_t *vpos;       // [nv] (p + 128), 9 bits per axis
    int *vcluster;        // [nv] rank of the cell among the occupied ones, -1: invalid
    uint32_t *bitmap, *prefix, *fblocks;
    SimplifyRow *rows;
    uint32_t n_rows;
    float *out_verts;
    int *source;
    uint32_t vcap;
    int *out_faces, *face_source;
    uint32_t fcap;
    uint32_t *counts;     // [0] clusters, [1] kept faces
};

__global__ __launch_bounds__(kSBlock) void simplify_mark_kernel(SimplifyArgs a)
{
    const size_t i = (size_t)blockIdx.x * kSBlock + threadIdx.x;
    int g[3], p[3];
    bool ok = i < (size_t)a.nv;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t = ok ? (a.verts[3 * i + k] - a.lo[k]) / a.cell : 0.0f;
        const float tf = floorf(t);
        const bool in = __builtin_isfinite(t) && tf >= 0.0f && tf < 2147483648.0f;
        g[k] = in ? (int)tf : 0;
        ok = ok && in && g[k] < a.G[k];
        const float r = fminf(fmaxf(rintf((t - tf - 0.5f) * 256.0f), -128.0f), 128.0f);
        p[k] = in ? (int)r : 0;
    }
    const int cell = ok ? (g[0] * a.G[1] + g[1]) * a.G[2] + g[2] : -1;
    if (i < (size_t)a.nv) {
        a.vcell[i] = cell;
        a.vpos[i] = ok ? (uint32_t)(p[0] + 128) | (uint32_t)(p[1] + 128) << 9 | (uint32_t)(p[2] + 128) << 18 : 0u;
    }
    // consecutive vertices of an extracted mesh share cells: one atomicOr per run of lanes with the same bitmap word, from the run's
    // last lane, with the bits of the whole run (segmented inclusive OR scan; every lane of the wave executes the shuffles)
    const int lane = threadIdx.x & 63, word = ok ? (int)((uint32_t)cell >> 5) : -1;
    uint32_t bits = ok ? 1u << (cell & 31) : 0u;
    const int prev = __shfl_up(word, 1, 64), next = __shfl_down(word, 1, 64);
    int head = lane == 0 || prev != word;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int head_up = __shfl_up(head, d, 64);
        const uint32_t up = __shfl_up(bits, d, 64);
        if (lane >= d && !head) bits |= up;
        if (lane >= d) head |= head_up;
    }
    if (word >= 0 && (lane == 63 || next != word)) atomicOr(&a.bitmap[word], bits);
}

struct ScanPopcount {
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const { return (uint32_t)__popc(v); }
};

// exclusive prefix sum of n values into out (in == out allowed), total to *total.  Value = ScanPopcount: the values are the
// popcounts of the words of in.
template <typename Value>
__global__ __launch_bounds__(kScanBlock) void simplify_scan_kernel(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *total)
{
    const uint32_t sum = block_exclusive_scan<uint32_t, Value>(in, out, n);
    if (threadIdx.x == kScanBlock - 1) *total = sum;
}

__global__ __launch_bounds__(kSBlock) void simplify_rank_kernel(SimplifyArgs a)
{
    const size_t i = (size_t)blockIdx.x * kSBlock + threadIdx.x;
    if (i >= (size_t)a.nv) return;
    const int cell = a.vcell[i];
    int c = -1;
    if (cell >= 0) {
        const uint32_t w = (uint32_t)cell >> 5;
        c = (int)(a.prefix[w] + (uint32_t)__popc(a.bitmap[w] & ((1u << (cell & 31)) - 1u)));
    }
    a.vcluster[i] = c;
}

// One face: does it count (indices in range, vertices valid, fp32 area neither 0 nor non-finite), its vertices and clusters,
// the cross product and its length.
struct SimplifyFace {
    int v[3], c[3];
    float N[3], L;
    bool counts;
};

__device__ __forceinline__ SimplifyFace simplify_face(const SimplifyArgs &a, size_t f)
{
    SimplifyFace r;
    r.counts = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.v[k] = a.faces[3 * f + k];
        const bool in = r.v[k] >= 0 && r.v[k] < a.nv;
        r.c[k] = in ? a.vcluster[r.v[k]] : -1;
        r.counts = r.counts && r.c[k] >= 0;
    }
    r.L = 0.0f;
    r.N[0] = r.N[1] = r.N[2] = 0.0f;
    if (r.counts) {
        float p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < 3; ++i) p[k][i] = a.verts[3 * (size_t)r.v[k] + i];
        const float e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const float e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        r.N[0] = e1[1] * e2[2] - e1[2] * e2[1];
        r.N[1] = e1[2] * e2[0] - e1[0] * e2[2];
        r.N[2] = e1[0] * e2[1] - e1[1] * e2[0];
        const float L2 = (r.N[0] * r.N[0] + r.N[1] * r.N[1]) + r.N[2] * r.N[2];
        r.counts = __builtin_isfinite(L2) && L2 > 0.0f;
        r.L = r.counts ? sqrtf(L2) : 0.0f;
    }
    return r;
}

__device__ __forceinline__ bool simplify_kept(const SimplifyFace &r)
{
    return r.counts && r.c[0] != r.c[1] && r.c[1] != r.c[2] && r.c[0] != r.c[2];
}

// block = 256 consecutive faces.  FILL = false: fblocks[b] = kept faces of the block; FILL = true: fblocks[b] holds the
// block's offset in the output and the kept faces go there in thread order.
template <bool FILL>
__global__ __launch_bounds__(kSBlock) void simplify_faces_kernel(SimplifyArgs a)
{
    __shared__ uint32_t wave_n[kSBlock / 64];
    const size_t f = (size_t)blockIdx.x * kSBlock + threadIdx.x;
    SimplifyFace r;
    bool keep = false;
    if (f < (size_t)a.nf) {
        r = simplify_face(a, f);
        keep = simplify_kept(r);
    }
    const unsigned long long votes = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = (uint32_t)__popcll(votes);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSBlock / 64; ++w) {
        if (w < wave) before += wave_n[w];
        total += wave_n[w];
    }
    if constexpr (!FILL) {
        if (threadIdx.x == 0) a.fblocks[blockIdx.x] = total;
    } else {
        if (!keep) return;
        const uint32_t slot = a.fblocks[blockIdx.x] + before + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
        if (slot >= a.fcap) return;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.out_faces[3 * (size_t)slot + k] = r.c[k];
        a.face_source[slot] = (int)f;
    }
}

// one thread per bitmap word: the cell index of every occupied cell into its row
__global__ __launch_bounds__(kSBlock) void simplify_cells_kernel(SimplifyArgs a)
{
    const uint32_t w = blockIdx.x * kSBlock + threadIdx.x;
    if (w >= a.words) return;
    uint32_t bits = a.bitmap[w], c = a.prefix[w];
    while (bits) {
        const int bit = __ffs(bits) - 1;
        bits &= bits - 1;
        if (c < a.n_rows) a.rows[c].cell = (int)(w * 32u + (uint32_t)bit);
        ++c;
    }
}

__device__ __forceinline__ void simplify_add(long long *p, long long v)
{
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);  // two's complement: the signed sum
}

__device__ __forceinline__ void simplify_unpack(uint32_t packed, int p[3])
{
    p[0] = (int)(packed & 511u) - 128;
    p[1] = (int)((packed >> 9) & 511u) - 128;
    p[2] = (int)((packed >> 18) & 511u) - 128;
}

// Sum of v[0..N) over every run of consecutive lanes with the same key, left in the LAST lane of the run (returns true there): a
// segmented inclusive scan with head flags, log2(64) steps of shuffles that every lane of the wave executes.  Integer sums: exact,
// so merging changes no result.  Lanes with key < 0 carry nothing.
template <int N>
__device__ __forceinline__ bool simplify_merge_runs(int key, long long (&v)[N])
{
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
    int head = lane == 0 || prev != key;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int head_up = __shfl_up(head, d, 64);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const long long up = __shfl_up(v[i], d, 64);
            if (lane >= d && !head) v[i] += up;
        }
        if (lane >= d) head |= head_up;
    }
    return key >= 0 && (lane == 63 || next != key);
}

__global__ __launch_bounds__(kSBlock) void simplify_vertex_sums_kernel(SimplifyArgs a)
{
    const size_t i = (size_t)blockIdx.x * kSBlock + threadIdx.x;
    int c = i < (size_t)a.nv ? a.vcluster[i] : -1;
    if ((uint32_t)c >= a.n_rows) c = -1;  // (invalid, or past the rows the caller gave)
    int p[3] = {0, 0, 0};
    if (c >= 0) simplify_unpack(a.vpos[i], p);
    long long v[4] = {p[0], p[1], p[2], c >= 0 ? 1 : 0};
    if (!simplify_merge_runs(c, v)) return;
    SimplifyRow *row = a.rows + c;
#pragma unroll
    for (int k = 0; k < 3; ++k) simplify_add(&row->S[k], v[k]);
    simplify_add(&row->cnt, v[3]);
}

__global__ __launch_bounds__(kSBlock) void simplify_face_sums_kernel(SimplifyArgs a)
{
    const size_t f = (size_t)blockIdx.x * kSBlock + threadIdx.x;
    SimplifyFace r;
    r.counts = false;
    if (f < (size_t)a.nf) r = simplify_face(a, f);
    long long n[3] = {0, 0, 0}, w = 0;
    if (r.counts) {
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = (long long)fminf(fmaxf(rintf(r.N[k] / r.L * 512.0f), -512.0f), 512.0f);
        w = (long long)fminf(fmaxf(rintf(0.5f * r.L / (a.cell * a.cell) * 1024.0f), 1.0f), 1024.0f);
    }
    const long long q[6] = {w * n[0] * n[0], w * n[0] * n[1], w * n[0] * n[2], w * n[1] * n[1], w * n[1] * n[2], w * n[2] * n[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int c = r.counts && (uint32_t)r.c[k] < a.n_rows ? r.c[k] : -1;
        long long v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (c >= 0) {
            int p[3];
            simplify_unpack(a.vpos[r.v[k]], p);
            const long long d = -(n[0] * p[0] + n[1] * p[1] + n[2] * p[2]);
#pragma unroll
            for (int i = 0; i < 6; ++i) v[i] = q[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) v[6 + i] = w * d * n[i];
        }
        if (!simplify_merge_runs(c, v)) continue;
        SimplifyRow *row = a.rows + c;
#pragma unroll
        for (int i = 0; i < 6; ++i) simplify_add(&row->A[i], v[i]);
#pragma unroll
        for (int i = 0; i < 3; ++i) simplify_add(&row->b[i], v[6 + i]);
    }
}

// one thread per cluster; f64, every operation rounded (no contraction), in the order DESIGN.md §19 and simplify_ref.py spell out
__global__ __launch_bounds__(kSBlock) void simplify_solve_kernel(SimplifyArgs a)
{
    const uint32_t c = blockIdx.x * kSBlock + threadIdx.x;
    const uint32_t nc = a.counts[0] < a.n_rows ? a.counts[0] : a.n_rows;
    if (c >= nc) return;
    SimplifyRow *row = a.rows + c;
    const long long lam_i = ((row->A[0] + row->A[3] + row->A[5]) >> 10) + 1;
    const double lam = (double)lam_i, cnt = (double)row->cnt;
    const double m[3] = {(double)row->S[0] / cnt, (double)row->S[1] / cnt, (double)row->S[2] / cnt};
    const double M00 = (double)row->A[0] + lam, M01 = (double)row->A[1], M02 = (double)row->A[2];
    const double M11 = (double)row->A[3] + lam, M12 = (double)row->A[4], M22 = (double)row->A[5] + lam;
    const double r0 = lam * m[0] - (double)row->b[0], r1 = lam * m[1] - (double)row->b[1], r2 = lam * m[2] - (double)row->b[2];
    const double c00 = M11 * M22 - M12 * M12, c01 = M02 * M12 - M01 * M22, c02 = M01 * M12 - M02 * M11;
    const double c11 = M00 * M22 - M02 * M02, c12 = M01 * M02 - M00 * M12, c22 = M00 * M11 - M01 * M01;
    const double det = (M00 * c00 + M01 * c01) + M02 * c02;
    double x[3] = {((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                   ((c02 * r0 + c12 * r1) + c22 * r2) / det};
    const bool solved = __builtin_isfinite(det) && det > 0.0 && __builtin_fabs(x[0]) <= 256.0 && __builtin_fabs(x[1]) <= 256.0 &&
                        __builtin_fabs(x[2]) <= 256.0;
    const int cell = row->cell;
    const int g[3] = {cell / (a.G[1] * a.G[2]), (cell / a.G[2]) % a.G[1], cell % a.G[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double xk = solved ? x[k] : m[k];
        const float pos = (float)((double)a.lo[k] + (((double)g[k] + 0.5) + xk / 256.0) * (double)a.cell);
        row->rep[k] = pos;
        if (c < a.vcap) a.out_verts[3 * (size_t)c + k] = pos;
    }
    row->key = ~0ull;
}

__global__ __launch_bounds__(kSBlock) void simplify_nearest_kernel(SimplifyArgs a)
{
    const size_t i = (size_t)blockIdx.x * kSBlock + threadIdx.x;
    if (i >= (size_t)a.nv) return;
    const int c = a.vcluster[i];
    if (c < 0 || (uint32_t)c >= a.n_rows) return;
    SimplifyRow *row = a.rows + c;
    const float dx = a.verts[3 * i] - row->rep[0], dy = a.verts[3 * i + 1] - row->rep[1], dz = a.verts[3 * i + 2] - row->rep[2];
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    atomicMin(&row->key, (unsigned long long)__float_as_uint(d2) << 32 | (unsigned long long)(uint32_t)i);
}

__global__ __launch_bounds__(kSBlock) void simplify_source_kernel(SimplifyArgs a)
{
    const uint32_t c = blockIdx.x * kSBlock + threadIdx.x;
    uint32_t nc = a.counts[0] < a.n_rows ? a.counts[0] : a.n_rows;
    nc = nc < a.vcap ? nc : a.vcap;
    if (c >= nc) return;
    a.source[c] = (int)(uint32_t)a.rows[c].key;
}

static inline uint32_t simplify_blocks(size_t n) { return (uint32_t)((n + kSBlock - 1) / kSBlock); }

// the workspace: vcell, vpos, vcluster [nv]; bitmap, prefix [words]; fblocks [ceil(nf / 256)] - all 4-byte words
static size_t simplify_layout(int nv, int nf, int GX, int GY, int GZ, size_t *words, size_t *fblocks)
{
    if (nv < 1 || nf < 0 || (int64_t)nf > kSMaxFaces || GX < 1 || GY < 1 || GZ < 1) return 0;
    if ((int64_t)GX * GY > 0x7fffffffLL || (int64_t)GX * GY * GZ > 0x7fffffffLL) return 0;
    const size_t w = ((size_t)GX * GY * GZ + 31) / 32, fb = ((size_t)nf + kSBlock - 1) / kSBlock;
    if (words) *words = w;
    if (fblocks) *fblocks = fb;
    return (3 * (size_t)nv + 2 * w + fb) * sizeof(uint32_t);
}

}  // namespace ojf

OJF_API size_t ojf_mesh_simplify_workspace_bytes(int nv, int nf, int GX, int GY, int GZ)
{
    return ojf::simplify_layout(nv, nf, GX, GY, GZ, nullptr, nullptr);
}

OJF_API size_t ojf_mesh_simplify_cluster_bytes(uint32_t nc)
{
    return sizeof(ojf::SimplifyRow) * (size_t)(nc ? nc : 1u);
}

OJF_API int ojf_mesh_simplify(const float *vertices, int nv, const int32_t *faces, int nf, const float *lo, float cell, int GX, int GY, int GZ,
                              int phases, void *workspace, size_t workspace_bytes, void *clusters, size_t clusters_bytes, float *out_vertices,
                              int32_t *source, uint32_t vertex_capacity, int32_t *out_faces, int32_t *face_source, uint32_t face_capacity,
                              uint32_t *counts, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_mesh_simplify";
    if (nv < 1) return refuse(who, "nv must be in 1..2^31-1");
    if (nf < 0 || (int64_t)nf > kSMaxFaces) return refuse(who, "nf must be in 0..2^24 (the integer sums are proved for that many faces)");
    if (GX < 1 || GY < 1 || GZ < 1 || (int64_t)GX * GY > 0x7fffffffLL || (int64_t)GX * GY * GZ > 0x7fffffffLL)
        return refuse(who, "the grid needs GX, GY, GZ >= 1 and GX*GY*GZ < 2^31");
    if (phases < 1 || phases > OJF_SIMPLIFY_ALL) return refuse(who, "phases must be a non-empty set of OJF_SIMPLIFY_* bits");
    if (!vertices || !lo || !workspace || !counts || (nf && !faces)) return refuse(who, "null pointer argument");
    if (!(cell > 0.0f) || !(cell < INFINITY)) return refuse(who, "cell must be > 0 and finite");
    if (!(fabsf(lo[0]) < INFINITY) || !(fabsf(lo[1]) < INFINITY) || !(fabsf(lo[2]) < INFINITY)) return refuse(who, "lo must be finite");
    size_t words = 0, fblocks = 0;
    const size_t need = simplify_layout(nv, nf, GX, GY, GZ, &words, &fblocks);
    if (workspace_bytes < need) return refuse(who, "workspace too small");
    const bool rows_used = phases & (OJF_SIMPLIFY_ACCUMULATE | OJF_SIMPLIFY_SOLVE | OJF_SIMPLIFY_NEAREST);
    if (rows_used && (!clusters || clusters_bytes < sizeof(SimplifyRow)))
        return refuse(who, "the ACCUMULATE, SOLVE and NEAREST phases need clusters_dev of ojf_mesh_simplify_cluster_bytes(counts[0])");
    if ((phases & (OJF_SIMPLIFY_SOLVE | OJF_SIMPLIFY_NEAREST)) && vertex_capacity && (!out_vertices || !source))
        return refuse(who, "vertex_capacity > 0 needs out_vertices_dev and source_dev (null pointer argument)");
    if ((phases & OJF_SIMPLIFY_FACES) && face_capacity && (!out_faces || !face_source))
        return refuse(who, "face_capacity > 0 needs out_faces_dev and face_source_dev (null pointer argument)");
    if (((uintptr_t)vertices & 3) || ((uintptr_t)faces & 3) || ((uintptr_t)workspace & 7) || ((uintptr_t)counts & 3) ||
        ((uintptr_t)out_vertices & 3) || ((uintptr_t)source & 3) || ((uintptr_t)out_faces & 3) || ((uintptr_t)face_source & 3))
        return refuse(who, "workspace_dev must be 8-byte, every array 4-byte aligned");
    if (rows_used && ((uintptr_t)clusters & 127)) return refuse(who, "clusters_dev must be 128-byte aligned");

    SimplifyArgs a;
    a.verts = vertices; a.faces = faces; a.nv = nv; a.nf = nf;
    a.lo[0] = lo[0]; a.lo[1] = lo[1]; a.lo[2] = lo[2]; a.cell = cell;
    a.G[0] = GX; a.G[1] = GY; a.G[2] = GZ;
    a.words = (uint32_t)words; a.fblocks_n = (uint32_t)fblocks;
    uint32_t *ws = static_cast<uint32_t *>(workspace);
    a.vcell = reinterpret_cast<int *>(ws);
    a.vpos = ws + (size_t)nv;
    a.vcluster = reinterpret_cast<int *>(ws + 2 * (size_t)nv);
    a.bitmap = ws + 3 * (size_t)nv;
    a.prefix = a.bitmap + words;
    a.fblocks = a.prefix + words;
    a.rows = static_cast<SimplifyRow *>(clusters);
    const size_t n_rows = rows_used ? clusters_bytes / sizeof(SimplifyRow) : 0;
    a.n_rows = n_rows > 0x7fffffffull ? 0x7fffffffu : (uint32_t)n_rows;
    a.out_verts = out_vertices; a.source = source; a.vcap = vertex_capacity;
    a.out_faces = out_faces; a.face_source = face_source; a.fcap = face_capacity;
    a.counts = counts;

    hipStream_t s = as_stream(stream);
    const dim3 block(kSBlock), vgrid(simplify_blocks((size_t)nv)), fgrid((uint32_t)fblocks), cgrid(simplify_blocks(a.n_rows));
    if (phases & OJF_SIMPLIFY_MARK) {
        OJF_HIP(hipMemsetAsync(a.bitmap, 0, words * sizeof(uint32_t), s));
        hipLaunchKernelGGL(simplify_mark_kernel, vgrid, block, 0, s, a);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_SIMPLIFY_SCAN) {
        hipLaunchKernelGGL(simplify_scan_kernel<ScanPopcount>, dim3(1), dim3(kScanBlock), 0, s, a.bitmap, a.prefix, a.words, counts);
        hipLaunchKernelGGL(simplify_rank_kernel, vgrid, block, 0, s, a);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_SIMPLIFY_COUNT) {
        if (nf) hipLaunchKernelGGL(simplify_faces_kernel<false>, fgrid, block, 0, s, a);
        hipLaunchKernelGGL(simplify_scan_kernel<ScanIdentity>, dim3(1), dim3(kScanBlock), 0, s, a.fblocks, a.fblocks, a.fblocks_n, counts + 1);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_SIMPLIFY_ACCUMULATE) {
        OJF_HIP(hipMemsetAsync(a.rows, 0, (size_t)a.n_rows * sizeof(SimplifyRow), s));
        hipLaunchKernelGGL(simplify_cells_kernel, dim3(simplify_blocks(words)), block, 0, s, a);
        hipLaunchKernelGGL(simplify_vertex_sums_kernel, vgrid, block, 0, s, a);
        if (nf) hipLaunchKernelGGL(simplify_face_sums_kernel, fgrid, block, 0, s, a);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_SIMPLIFY_SOLVE) {
        hipLaunchKernelGGL(simplify_solve_kernel, cgrid, block, 0, s, a);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_SIMPLIFY_NEAREST) {
        hipLaunchKernelGGL(simplify_nearest_kernel, vgrid, block, 0, s, a);
        if (vertex_capacity) hipLaunchKernelGGL(simplify_source_kernel, dim3(simplify_blocks(vertex_capacity < a.n_rows ? vertex_capacity : a.n_rows)), block, 0, s, a);
        OJF_HIP(hipGetLastError());
    }
    if ((phases & OJF_SIMPLIFY_FACES) && nf && face_capacity) {
        hipLaunchKernelGGL(simplify_faces_kernel<true>, fgrid, block, 0, s, a);
        OJF_HIP(hipGetLastError());
    }
    return 0;
}
