// CONNECTED COMPONENTS of a volume: the one volume operator whose answer at a voxel depends on voxels arbitrarily far away.
// Floater removal (Database.filter_components) and 3-D instances of the label volume (Database.instances) are built on it.
// Own definition (the reference has no such step); tests/components_ref.py restates it in numpy without bricks and the GPU
// tests pin the kernels to it bit for bit.
//
// Normative definition.  Volumes are [X,Y,Z] with z contiguous; the linear index of a voxel is v = (x·Y + y)·Z + z.
//   mask u8 (or absent): a voxel is foreground when its byte is non-zero; absent: every voxel is foreground.
//   keys u8 (or absent): two neighbouring foreground voxels are joined only when their key bytes are equal; absent: always.
//   connectivity 6: neighbours share a face; 26: the full 3x3x3 neighbourhood.  Components are the classes of the
//     transitive closure of "joined".
//   labels i32 [X,Y,Z]: -1 on the background, else the smallest linear index of the voxel's component (its root).
//   the list, in ascending order of root, n entries: roots i32, sizes i32 (voxels), keys u8 (the key byte at the root, 0
//     without keys), boxes i32[6] = (x0, y0, z0, x1, y1, z1), the inclusive minimum and maximum of each coordinate.
//   ids i32 [X,Y,Z]: -1 on the background, else the rank 0..n-1 of the voxel's component in the list.
// All of it is a function of the input alone: brick shape, launch order and the order in which atomics arrive show nowhere.
//
// Observed mask (ojf_volume_observed_mask): foreground when fp32(weight) > 0 and the TSDF value is not a NaN - the mesh
//   extractor's notion of an observed voxel (a NaN, negative or -0 weight is unobserved, the smallest subnormal observed) -
//   and, with a band, |fp32(tsdf)| < band.
// Removal (ojf_volume_components_apply): where ids[v] names a component whose keep flag is 0: tsdf = init_value (rounded to
//   fp16 as ojf_volume_filter rounds it), weight = 0.  Voxels of kept components and background voxels are not written.
//
// Shape.  The volume is cut into bricks of 4 x 4 x 64 voxels (x, y, z): a wave reads one 64-byte z-row of the u8 inputs,
// a block of 256 lanes owns the brick's 1024 voxels, four x-slices each, and what a brick-local component has to hand on -
// its size (<= 1024) and its box inside the brick (2 + 2 + 6 bits, twice) - fits 30 bits of one i32 per voxel.
//   brick  (comp_brick_kernel): union-find in LDS.  Every foreground voxel unites itself with those of its 13 (3 for
//     connectivity 6) lexicographically smaller neighbours that lie in the same brick, are foreground and hold its key:
//     find by pointer chasing, hook the larger root under the smaller one with an LDS atomicMin.  The brick-local index
//     orders the voxels as the linear index does, so the brick-local root is the smallest linear index of the brick-local
//     component.  Sizes come from an LDS atomicAdd at the root, boxes from LDS atomicOr of occupancy bits (4 + 4 bits of
//     x and y, 64 of z): count-leading/trailing-zeros turn them into minima and maxima.  Out: labels[v] = linear index of
//     the brick-local root (-1 background) and stats[v] = the packed size and box at brick-local roots, -1 elsewhere.
//     No communication between workgroups.
//   seam   (comp_seam_kernel): one lane per voxel; those on a brick's shell look at the same 13 (3) smaller neighbours and
//     unite across the pairs that straddle two bricks - faces, and for 26 the edge and corner diagonals - in the labels
//     array in global memory.  Workgroups on all eight XCDs rewrite the same words here, the XCDs' L2s are not coherent
//     with each other and a CU's L1 is never refreshed by another CU's stores: EVERY access to the labels array in this
//     kernel is an agent-scope atomic (relaxed load, fetch-min), which is served where all CUs agree.  A stale plain load
//     could present a root that has long been hooked, or an edge that was replaced.  Hooking puts the larger root under
//     the smaller, so parents only ever decrease and the final root is the component's smallest index.  The only loops are
//     the find loop (strictly decreasing indices) and the retry of a hook whose fetch-min found that another lane had
//     hooked the same root first - it then goes on uniting with what it found.  No lane waits for another workgroup.
//   flatten (comp_flatten_kernel), after the kernel boundary: labels[v] = find(v); a reader that meets a voxel already
//     flattened meets an ancestor all the same.
//   rank   : comp_count_kernel counts the roots (labels[v] == v) of every run of 1024 voxels, comp_scan_kernel makes the
//     counts exclusive offsets (one block: ojf_blocks.h), comp_rank_kernel writes each root's rank at ids[root]
//     and comp_gather_kernel ids[v] = ids[labels[v]].
//   list   : comp_list_kernel writes roots and keys and adds the brick-local figures to the entry of their component: at
//     most one integer atomicAdd, three atomicMin and three atomicMax per brick-local component, never one per voxel (the
//     room's main component has millions of voxels and one counter word) - and fewer where a lane, and then its block,
//     can add up brick-local components of one component first (a single word takes ~88 atomics/us: with one set per
//     brick-local component this pass alone took 3.9 ms on a 256^3 serpentine).  Integer atomics only: the sums and
//     extrema do not depend on their order or on who added what up.  The list phase reads only labels, ids, the keys
//     and the workspace: it may run in a later call, with a list sized by the n the first call returned (capacity /
//     count as in ojf_mesh_extract).
#include "ojf_blocks.h"

namespace ojf {

constexpr int kCBx = 4, kCBy = 4, kCBz = 64;       // the brick
constexpr int kCBrick = kCBx * kCBy * kCBz;        // 1024 voxels
constexpr int kCBlock = 256;                       // lanes per block, everywhere in this file
constexpr int kCRun = 1024;                        // voxels per block of the root count / rank kernels

#define OJF_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct CompArgs {
    const uint8_t *mask, *keys;  // either may be NULL
    int X, Y, Z;
    int nbx, nby, nbz;
    int conn;      // 6 or 26
    int *labels;   // [X,Y,Z]
    int *stats;    // [X,Y,Z], the workspace
};

// Offset o of the 13 lexicographically negative ones of the 3x3x3 neighbourhood; false when connectivity 6 leaves it out.
__device__ __forceinline__ bool comp_offset(int o, int conn, int &dx, int &dy, int &dz)
{
    if (o < 9) { dx = -1; dy = o / 3 - 1; dz = o % 3 - 1; }
    else if (o < 12) { dx = 0; dy = -1; dz = o - 10; }
    else { dx = 0; dy = 0; dz = -1; }
    return conn == 26 || (dx != 0) + (dy != 0) + (dz != 0) == 1;
}

// ---- brick -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int *L, int a)
{
    int p;
    while ((p = __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != a) a = p;
    return a;
}

__device__ __forceinline__ void lds_unite(int *L, int a, int b)
{
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(L + a, b);  // hook root a under the smaller b
        if (old == a) return;
        a = old;  // another lane hooked a first (under old < a): old and b are still to be united
    }
}

__global__ __launch_bounds__(kCBlock) void comp_brick_kernel(CompArgs a)
{
    __shared__ int L[kCBrick];
    __shared__ short K[kCBrick];                  // the key of a foreground voxel, -1: background or outside the volume
    __shared__ int cnt[kCBrick];
    __shared__ unsigned int occ_xy[kCBrick];      // bit lx, bit 4 + ly
    __shared__ unsigned long long occ_z[kCBrick];  // bit lz
    const uint32_t b = blockIdx.x;
    const int bz = (int)(b % (uint32_t)a.nbz);
    const int by = (int)((b / (uint32_t)a.nbz) % (uint32_t)a.nby);
    const int bx = (int)(b / ((uint32_t)a.nbz * (uint32_t)a.nby));
    const int t = threadIdx.x, lz = t & (kCBz - 1), ly = t >> 6;  // the lane's voxels: (i, ly, lz), i = 0..3, l = 256 i + t
    const int gy = by * kCBy + ly, gz = bz * kCBz + lz;
    const bool row_in = gy < a.Y && gz < a.Z;
#pragma unroll
    for (int i = 0; i < kCBx; ++i) {
        const int l = i * kCBlock + t, gx = bx * kCBx + i;
        int k = -1;
        if (row_in && gx < a.X) {
            const size_t g = ((size_t)gx * a.Y + gy) * a.Z + gz;
            if (!a.mask || a.mask[g] != 0) k = a.keys ? (int)a.keys[g] : 0;
        }
        K[l] = (short)k;
        L[l] = l;
        cnt[l] = 0;
        occ_xy[l] = 0u;
        occ_z[l] = 0ull;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kCBx; ++i) {
        const int l = i * kCBlock + t;
        const int k = K[l];
        if (k < 0) continue;
        for (int o = 0; o < 13; ++o) {
            int dx, dy, dz;
            if (!comp_offset(o, a.conn, dx, dy, dz)) continue;
            const int nx = i + dx, ny = ly + dy, nz = lz + dz;
            if ((unsigned)nx >= (unsigned)kCBx || (unsigned)ny >= (unsigned)kCBy || (unsigned)nz >= (unsigned)kCBz) continue;
            const int nl = (nx * kCBy + ny) * kCBz + nz;
            if (K[nl] == k) lds_unite(L, l, nl);
        }
    }
    __syncthreads();
    int r[kCBx];
#pragma unroll
    for (int i = 0; i < kCBx; ++i) {
        const int l = i * kCBlock + t;
        r[i] = K[l] >= 0 ? lds_find(L, l) : -1;  // (nothing writes L any more)
        if (r[i] >= 0) {
            atomicAdd(cnt + r[i], 1);
            atomicOr(occ_xy + r[i], (1u << i) | (1u << (kCBx + ly)));
            atomicOr(occ_z + r[i], 1ull << lz);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kCBx; ++i) {
        const int l = i * kCBlock + t, gx = bx * kCBx + i;
        if (!(row_in && gx < a.X)) continue;
        const size_t g = ((size_t)gx * a.Y + gy) * a.Z + gz;
        int label = -1, packed = -1;
        if (r[i] >= 0) {
            const int rx = r[i] >> 8, ry = (r[i] >> 6) & 3, rz = r[i] & 63;
            label = (int)(((size_t)(bx * kCBx + rx) * a.Y + (by * kCBy + ry)) * a.Z + (bz * kCBz + rz));
            if (r[i] == l) {
                const unsigned int xs = occ_xy[l] & 15u, ys = occ_xy[l] >> 4;
                const unsigned long long zs = occ_z[l];
                const int x0 = __builtin_ctz(xs), x1 = 31 - __builtin_clz(xs), y0 = __builtin_ctz(ys), y1 = 31 - __builtin_clz(ys);
                const int z0 = __builtin_ctzll(zs), z1 = 63 - __builtin_clzll(zs);
                packed = (cnt[l] - 1) | (x0 << 10) | (x1 << 12) | (y0 << 14) | (y1 << 16) | (z0 << 18) | (z1 << 24);
            }
        }
        a.labels[g] = label;
        a.stats[g] = packed;
    }
}

// ---- seam ------------------------------------------------------------------------------------------------------------
// Every access to the parent array goes through these two.
__device__ __forceinline__ int agent_find(int *parent, int a)
{
    int p;
    while ((p = __hip_atomic_load(parent + a, OJF_RLX_AGENT)) != a) a = p;
    return a;
}

__device__ __forceinline__ void agent_unite(int *parent, int a, int b)
{
    for (;;) {
        a = agent_find(parent, a);
        b = agent_find(parent, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = __hip_atomic_fetch_min(parent + a, b, OJF_RLX_AGENT);
        if (old == a) return;
        a = old;  // as in lds_unite: the lane that got there first made progress; go on from what it left
    }
}

__global__ __launch_bounds__(kCBlock) void comp_seam_kernel(CompArgs a, uint32_t total)
{
    const uint32_t v = blockIdx.x * (uint32_t)kCBlock + threadIdx.x;
    if (v >= total) return;
    const int z = (int)(v % (uint32_t)a.Z);
    const int y = (int)((v / (uint32_t)a.Z) % (uint32_t)a.Y);
    const int x = (int)(v / ((uint32_t)a.Z * (uint32_t)a.Y));
    const int lx = x & (kCBx - 1), ly = y & (kCBy - 1), lz = z & (kCBz - 1);
    if (lx > 0 && lx < kCBx - 1 && ly > 0 && ly < kCBy - 1 && lz > 0 && lz < kCBz - 1) return;  // every neighbour is in the brick
    if (a.mask && a.mask[v] == 0) return;
    const int k = a.keys ? (int)a.keys[v] : 0;
    for (int o = 0; o < 13; ++o) {
        int dx, dy, dz;
        if (!comp_offset(o, a.conn, dx, dy, dz)) continue;
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        if ((unsigned)nx >= (unsigned)a.X || (unsigned)ny >= (unsigned)a.Y || (unsigned)nz >= (unsigned)a.Z) continue;
        if ((nx >> 2) == (x >> 2) && (ny >> 2) == (y >> 2) && (nz >> 6) == (z >> 6)) continue;  // the brick pass joined these
        const size_t u = ((size_t)nx * a.Y + ny) * a.Z + nz;
        if (a.mask && a.mask[u] == 0) continue;
        if (a.keys && (int)a.keys[u] != k) continue;
        agent_unite(a.labels, (int)v, (int)u);
    }
}

__global__ __launch_bounds__(kCBlock) void comp_flatten_kernel(int *labels, uint32_t total)
{
    const uint32_t v = blockIdx.x * (uint32_t)kCBlock + threadIdx.x;
    if (v >= total) return;
    const int p = __hip_atomic_load(labels + v, OJF_RLX_AGENT);
    if (p < 0) return;
    __hip_atomic_store(labels + v, agent_find(labels, p), OJF_RLX_AGENT);
}

// ---- rank ------------------------------------------------------------------------------------------------------------
// Block b owns voxels [1024 b, 1024 b + 1024): lane t the voxels 1024 b + 256 i + t, i = 0..3.
__global__ __launch_bounds__(kCBlock) void comp_count_kernel(const int *labels, uint32_t total, uint32_t *counts)
{
    int n = 0;
#pragma unroll
    for (int i = 0; i < kCRun / kCBlock; ++i) {
        const uint64_t v = (uint64_t)blockIdx.x * kCRun + (uint32_t)(i * kCBlock) + threadIdx.x;
        n += __syncthreads_count(v < total && labels[v] == (int)v);
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = (uint32_t)n;
}

// exclusive prefix sum of counts[0..n) in place, the total to *total_ws and *count_out
__global__ __launch_bounds__(kScanBlock) void comp_scan_kernel(uint32_t *counts, uint32_t n, uint32_t *total_ws, uint32_t *count_out)
{
    const uint32_t total = block_exclusive_scan<uint32_t>(counts, counts, n);
    if (threadIdx.x == kScanBlock - 1) {
        *total_ws = total;
        *count_out = total;
    }
}

__global__ __launch_bounds__(kCBlock) void comp_rank_kernel(const int *labels, uint32_t total, const uint32_t *offsets, int *ids)
{
    __shared__ uint32_t wave_n[kCBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t run = offsets[blockIdx.x];
#pragma unroll
    for (int i = 0; i < kCRun / kCBlock; ++i) {
        const uint64_t v = (uint64_t)blockIdx.x * kCRun + (uint32_t)(i * kCBlock) + threadIdx.x;
        const bool root = v < total && labels[v] == (int)v;
        const unsigned long long m = __ballot(root);
        if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kCBlock / 64; ++w) {
            if (w < wave) before += wave_n[w];
            all += wave_n[w];
        }
        if (root) ids[v] = (int)(run + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
        run += all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kCBlock) void comp_gather_kernel(const int *labels, uint32_t total, int *ids)
{
    const uint32_t v = blockIdx.x * (uint32_t)kCBlock + threadIdx.x;
    if (v >= total) return;
    const int l = labels[v];
    if (l != (int)v) ids[v] = l < 0 ? -1 : ids[l];  // (a root keeps the rank comp_rank_kernel gave it)
}

// ---- list ------------------------------------------------------------------------------------------------------------
struct ListArgs {
    const int *labels, *ids, *stats;
    const uint8_t *keys;
    const uint32_t *n;  // the number of components, in the workspace
    int X, Y, Z;
    int *roots, *sizes, *boxes;
    uint8_t *keys_out;
    uint32_t cap;
};

__global__ __launch_bounds__(kCBlock) void comp_list_init_kernel(ListArgs a)
{
    const uint32_t i = blockIdx.x * (uint32_t)kCBlock + threadIdx.x;
    if (i >= a.cap || i >= *a.n) return;
    a.sizes[i] = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        a.boxes[6 * (size_t)i + m] = 0x7fffffff;
        a.boxes[6 * (size_t)i + 3 + m] = -1;
    }
}

struct ListSum {  // the figures of some brick-local components of one component
    int size, lo[3], hi[3];
};

__device__ __forceinline__ void list_add(const ListArgs &a, uint32_t rank, const ListSum &s)
{
    int *box = a.boxes + 6 * (size_t)rank;
    atomicAdd(a.sizes + rank, s.size);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        atomicMin(box + m, s.lo[m]);
        atomicMax(box + 3 + m, s.hi[m]);
    }
}

// Grid-stride over the voxels; the work is at the brick-local roots.  A lane keeps the sum of the brick-local components it
// meets for as long as they belong to one component and hands it on when the component changes; at the end the block adds
// up, in LDS, the sums of the lanes that hold the component of the lane with the largest one.  Where one component owns
// most of the volume (the room) its counter words receive one atomic per block instead of one per brick-local component;
// where every voxel is its own component nothing is saved and nothing is lost.
__global__ __launch_bounds__(kCBlock) void comp_list_kernel(ListArgs a, uint32_t total)
{
    __shared__ unsigned long long pick;  // max of (size << 32) | rank over the lanes
    __shared__ int acc[7];
    constexpr uint32_t kNone = 0xffffffffu;
    uint32_t held = kNone;
    ListSum sum;
    if (threadIdx.x == 0) {
        pick = 0ull;
        acc[0] = 0;
        for (int m = 0; m < 3; ++m) { acc[1 + m] = 0x7fffffff; acc[4 + m] = -1; }
    }
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * kCBlock;
    for (uint64_t v = (uint64_t)blockIdx.x * kCBlock + threadIdx.x; v < total; v += step) {
        const int p = a.stats[v];
        if (p < 0) continue;  // not a brick-local root (every root is one)
        const uint32_t rank = (uint32_t)a.ids[v];
        if (rank >= a.cap) continue;
        if (a.labels[v] == (int)v) {
            a.roots[rank] = (int)v;
            a.keys_out[rank] = a.keys ? a.keys[v] : (uint8_t)0;
        }
        const int z = (int)((uint32_t)v % (uint32_t)a.Z);
        const int y = (int)(((uint32_t)v / (uint32_t)a.Z) % (uint32_t)a.Y);
        const int x = (int)((uint32_t)v / ((uint32_t)a.Z * (uint32_t)a.Y));
        const int ox = x & ~(kCBx - 1), oy = y & ~(kCBy - 1), oz = z & ~(kCBz - 1);
        ListSum one;
        one.size = (p & 1023) + 1;
        one.lo[0] = ox + ((p >> 10) & 3); one.hi[0] = ox + ((p >> 12) & 3);
        one.lo[1] = oy + ((p >> 14) & 3); one.hi[1] = oy + ((p >> 16) & 3);
        one.lo[2] = oz + ((p >> 18) & 63); one.hi[2] = oz + ((p >> 24) & 63);
        if (rank != held) {
            if (held != kNone) list_add(a, held, sum);
            held = rank;
            sum = one;
        } else {
            sum.size += one.size;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                sum.lo[m] = min(sum.lo[m], one.lo[m]);
                sum.hi[m] = max(sum.hi[m], one.hi[m]);
            }
        }
    }
    if (held != kNone) atomicMax(&pick, ((unsigned long long)(uint32_t)sum.size << 32) | held);
    __syncthreads();
    const unsigned long long picked = pick;
    if (picked == 0ull) return;  // no lane holds anything (a sum has a size >= 1)
    const uint32_t shared_rank = (uint32_t)picked;
    if (held != kNone) {
        if (held == shared_rank) {
            atomicAdd(acc, sum.size);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                atomicMin(acc + 1 + m, sum.lo[m]);
                atomicMax(acc + 4 + m, sum.hi[m]);
            }
        } else {
            list_add(a, held, sum);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ListSum all;
        all.size = acc[0];
#pragma unroll
        for (int m = 0; m < 3; ++m) { all.lo[m] = acc[1 + m]; all.hi[m] = acc[4 + m]; }
        list_add(a, shared_rank, all);
    }
}

// ---- observed mask, removal --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t observed(uint16_t t, uint16_t w, bool use_band, float band)
{
    return (voxel_observed(t, w) && (!use_band || fabsf(h2f(t)) < band)) ? 1u : 0u;
}

__global__ __launch_bounds__(kCBlock) void observed_mask_kernel(const uint16_t *tsdf, const uint16_t *wgt, size_t n, int use_band, float band,
                                                                uint8_t *mask)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const bool aligned = (((uintptr_t)tsdf | (uintptr_t)wgt) & 15) == 0 && ((uintptr_t)mask & 7) == 0;
    const size_t nvec = aligned ? n / 8 : 0;
    for (size_t i = tid; i < nvec; i += step) {
        uint32_t tq[4], wq[4], out[2] = {0u, 0u};
        load8(tsdf, i, tq);
        load8(wgt, i, wq);
#pragma unroll
        for (int e = 0; e < 8; ++e) set8(out, e, observed((uint16_t)get16(tq, e), (uint16_t)get16(wq, e), use_band != 0, band));
        reinterpret_cast<uint2 *>(mask)[i] = make_uint2(out[0], out[1]);
    }
    for (size_t i = nvec * 8 + tid; i < n; i += step) mask[i] = (uint8_t)observed(tsdf[i], wgt[i], use_band != 0, band);
}

__global__ __launch_bounds__(kCBlock) void components_apply_kernel(const int *ids, const uint8_t *keep, uint32_t n_components, uint16_t *tsdf,
                                                                   uint16_t *wgt, size_t n, uint16_t init_bits)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < n; i += step) {
        const int id = ids[i];
        if (id >= 0 && (uint32_t)id < n_components && keep[id] == 0) {
            tsdf[i] = init_bits;
            wgt[i] = 0;
        }
    }
}

static inline uint32_t comp_runs(uint32_t total) { return (total + kCRun - 1) / kCRun; }

}  // namespace ojf

OJF_API size_t ojf_volume_components_workspace_bytes(int X, int Y, int Z)
{
    if (!ojf::volume_size_ok(X, Y, Z)) return 0;
    const uint32_t total = (uint32_t)((int64_t)X * Y * Z);
    // the brick-local figures (i32 per voxel), the root counts / offsets (u32 per run of 1024 voxels), n (u32), to 8 bytes
    return (((size_t)total + ojf::comp_runs(total) + 1) * sizeof(uint32_t) + 7) & ~(size_t)7;
}

OJF_API int ojf_volume_components(const uint8_t *mask, const uint8_t *keys, int X, int Y, int Z, int connectivity, int phases, void *workspace,
                                  size_t workspace_bytes, int32_t *labels, int32_t *ids, int32_t *roots, int32_t *sizes, uint8_t *list_keys,
                                  int32_t *boxes, uint32_t capacity, uint32_t *count, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_volume_components";
    if (!workspace || !labels || !ids) return refuse(who, "null pointer argument");
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    if (connectivity != 6 && connectivity != 26) return refuse(who, "connectivity must be 6 or 26");
    if (phases < 1 || phases > OJF_COMPONENTS_ALL) return refuse(who, "phases must be a non-empty set of OJF_COMPONENTS_* bits");
    if (capacity == 0) phases &= ~OJF_COMPONENTS_LIST;
    if (phases == 0) return refuse(who, "capacity 0 runs no list phase");
    if ((phases & OJF_COMPONENTS_RANK) && !count) return refuse(who, "null pointer argument: count_dev");
    if ((phases & OJF_COMPONENTS_LIST) && (!roots || !sizes || !list_keys || !boxes))
        return refuse(who, "null pointer argument: the list arrays with capacity > 0");
    if (workspace_bytes < ojf_volume_components_workspace_bytes(X, Y, Z)) return refuse(who, "workspace too small");
    if (((uintptr_t)workspace & 7) || ((uintptr_t)labels & 3) || ((uintptr_t)ids & 3) || ((uintptr_t)roots & 3) || ((uintptr_t)sizes & 3) ||
        ((uintptr_t)boxes & 3) || ((uintptr_t)count & 3))
        return refuse(who, "workspace_dev must be 8-byte, the i32 and u32 arrays 4-byte aligned");

    const uint32_t total = (uint32_t)((int64_t)X * Y * Z), runs = comp_runs(total);
    int *const stats = reinterpret_cast<int *>(workspace);
    uint32_t *const counts = reinterpret_cast<uint32_t *>(workspace) + total, *const n_ws = counts + runs;
    CompArgs a;
    a.mask = mask; a.keys = keys;
    a.X = X; a.Y = Y; a.Z = Z;
    a.nbx = (X + kCBx - 1) / kCBx; a.nby = (Y + kCBy - 1) / kCBy; a.nbz = (Z + kCBz - 1) / kCBz;
    a.conn = connectivity;
    a.labels = labels; a.stats = stats;
    const uint64_t bricks = (uint64_t)a.nbx * a.nby * a.nbz;  // <= 2^31 / ... : X·Y·Z < 2^31 and every brick holds a voxel
    const dim3 per_voxel((total + kCBlock - 1) / kCBlock), block(kCBlock);
    hipStream_t s = as_stream(stream);
    if (phases & OJF_COMPONENTS_BRICK) {
        hipLaunchKernelGGL(comp_brick_kernel, dim3((uint32_t)bricks), block, 0, s, a);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_COMPONENTS_SEAM) {
        hipLaunchKernelGGL(comp_seam_kernel, per_voxel, block, 0, s, a, total);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_COMPONENTS_FLATTEN) {
        hipLaunchKernelGGL(comp_flatten_kernel, per_voxel, block, 0, s, labels, total);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_COMPONENTS_RANK) {
        hipLaunchKernelGGL(comp_count_kernel, dim3(runs), block, 0, s, labels, total, counts);
        hipLaunchKernelGGL(comp_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, counts, runs, n_ws, count);
        hipLaunchKernelGGL(comp_rank_kernel, dim3(runs), block, 0, s, labels, total, counts, ids);
        hipLaunchKernelGGL(comp_gather_kernel, per_voxel, block, 0, s, labels, total, ids);
        OJF_HIP(hipGetLastError());
    }
    if (phases & OJF_COMPONENTS_LIST) {
        ListArgs l;
        l.labels = labels; l.ids = ids; l.stats = stats; l.keys = keys; l.n = n_ws;
        l.X = X; l.Y = Y; l.Z = Z;
        l.roots = roots; l.sizes = sizes; l.boxes = boxes; l.keys_out = list_keys; l.cap = capacity;
        const uint32_t cap_blocks = (uint32_t)(((uint64_t)(capacity < total ? capacity : total) + kCBlock - 1) / kCBlock);
        hipLaunchKernelGGL(comp_list_init_kernel, dim3(cap_blocks), block, 0, s, l);
        hipLaunchKernelGGL(comp_list_kernel, dim3(stream_grid(total, kCBlock)), block, 0, s, l, total);
        OJF_HIP(hipGetLastError());
    }
    return 0;
}

OJF_API int ojf_volume_observed_mask(const uint16_t *tsdf, const uint16_t *wgt, size_t n, int use_band, float band, uint8_t *mask,
                                     ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_volume_observed_mask";
    if (!tsdf || !wgt || !mask) return refuse(who, "null pointer argument");
    if (n == 0 || n > 0x7fffffffULL) return refuse(who, "the voxel count must be in 1..2^31-1");
    if (use_band && !(band > 0.0f)) return refuse(who, "band must be > 0 (a NaN is refused)");
    if (((uintptr_t)tsdf & 1) || ((uintptr_t)wgt & 1)) return refuse(who, "tsdf_dev and weights_dev must be 2-byte aligned");
    hipLaunchKernelGGL(observed_mask_kernel, dim3(stream_grid(n / 8 + 1, kCBlock)), dim3(kCBlock), 0, as_stream(stream), tsdf, wgt, n, use_band, band,
                       mask);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_volume_components_apply(const int32_t *ids, const uint8_t *keep, uint32_t n_components, uint16_t *tsdf, uint16_t *wgt, size_t n,
                                        float init_value, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_volume_components_apply";
    if (!ids || !tsdf || !wgt || (!keep && n_components)) return refuse(who, "null pointer argument");
    if (n == 0 || n > 0x7fffffffULL) return refuse(who, "the voxel count must be in 1..2^31-1");
    if (((uintptr_t)ids & 3) || ((uintptr_t)tsdf & 1) || ((uintptr_t)wgt & 1)) return refuse(who, "ids_dev must be 4-byte, the volumes 2-byte aligned");
    if (n_components == 0) return 0;  // nothing to remove
    const _Float16 hv = (_Float16)init_value;
    uint16_t bits;
    __builtin_memcpy(&bits, &hv, 2);
    hipLaunchKernelGGL(components_apply_kernel, dim3(stream_grid(n, kCBlock)), dim3(kCBlock), 0, as_stream(stream), ids, keep, n_components, tsdf, wgt,
                       n, bits);
    OJF_HIP(hipGetLastError());
    return 0;
}
