// RELOC: keyframe relocalisation by randomised ferns (Glocker et al. 2013, "Real-time RGB-D camera relocalization", as used
// by InfiniTAM and ElasticFusion) - a constant-time code per frame, a store of keyframe codes with their poses on the device,
// and the nearest-keyframe search.  Own definition (the reference takes every pose from its dataset); tests/reloc_ref.py
// restates it in numpy and the GPU tests pin the kernels to it bit for bit.
//
// Normative definition.
//
//   Inputs per frame: depth f32 [h,w]; mask u8 [h,w] or NULL; image u8 [h,w,4] (color.pack_image: R, G, B, padding) or NULL.
//
//   Pixel validity and quantisation.  A pixel is valid when its mask byte != 0 (if a mask is given), its depth is finite and
//   0 < depth < 64.  q = (u32) rintf(depth * 1024.f)  (round to nearest even; the product is exact).
//
//   Code image.  cell c in 1..64; CH = h / c, CW = w / c by integer division, trailing rows and columns are ignored, CH >= 1,
//   CW >= 1 (and CH * CW <= 1024 here: the code image lives in LDS).  Cell (i, j) covers rows i*c .. i*c + c - 1 and
//   columns j*c .. j*c + c - 1; its index is i * CW + j.
//     channel 0: S = the exact u32 sum of q over the cell's valid pixels, n their count.  If 2n >= c*c the cell is valid and
//       its value is ((float)S / (float)n) * 2^-10; otherwise the cell is invalid and its value is 0.
//     channels 1..3 (only with an image): (float)S_byte / (float)(c*c) with S_byte the u32 sum of the R, G, B bytes over all
//       pixels of the cell; always valid.  Without an image they are 0.
//   Integer sums: the result does not depend on the order of summation.
//
//   Ferns.  M ferns, M a multiple of 8, 8 <= M <= 4096.  Fern m has 4 decisions j = 0..3 (cell index i32, channel u8 0..3,
//   threshold f32), at [m][j] of three arrays.  bit j = value(cell, channel) > threshold (strict; a NaN threshold gives 0), and
//   for channel 0 also that the cell is valid; a cell index outside 0..CH*CW-1 gives bit 0, of a channel only its low two
//   bits count.  The fern's code is bit0 | bit1 << 1 | bit2 << 2 | bit3 << 3.  Fern m sits in word m / 8 at bits
//   4*(m%8) .. +3: M/8 u32 words per frame.
//
//   Dissimilarity of two codes: the number of ferns whose nibbles differ, 0..M.  The key of keyframe i against a query:
//   (u64)count << 32 | i.
//
//   Query: the k (1..16) smallest keys over the first `count` keyframes of the store, ascending - equal codes come out
//   smallest index first; places beyond `count` hold all-ones.  `count` is read on the device and clamped to 0..capacity.
//
//   Insert: the n frames of a call are processed in order.  best = the smallest key over the store as it stands, frames
//   added earlier in the same call included; all-ones when the store is empty.  A frame is wanted when `force`, or the store
//   is empty, or best's count > min_differ.  Flags: 0 not wanted (too similar); 2 wanted but the store is full
//   (count == capacity; nothing is written); 1 added - the frame takes slot `count`, its M/8 code words and its f64[12]
//   pose are copied, and count becomes count + 1.  best and the flag of every frame are written out.
//
//   Store (device memory the caller owns): codes u32 [capacity][M/8], poses f64 [capacity][12], count i32 [1].
//
// Shape.  The entry points take no workspace, which decides the shapes.
//   encode: one launch, one workgroup of 1024 lanes per frame.  The cells' sums are LDS integer atomics (one 64-bit add of
//     n << 32 | S per lane and one of R | G << 21 | B << 42): where the frame, mask and image are 16-byte aligned, w % 4 == 0
//     and c % 4 == 0 a lane takes four neighbouring pixels of one cell with one 16-byte load and adds their sum once; any
//     other case takes one pixel per lane.  Both give the same bits (integer sums).  The code image never leaves LDS unless
//     it is asked for; the M ferns are then evaluated from it, one fern per lane, and eight neighbouring lanes combine their
//     nibbles into a word by three xor-shuffles.  One CU per frame: a single frame is bound by that CU's load latency, not by
//     bytes (DESIGN.md section 26 has the figures).
//   query: grid (B, n), 16 waves per workgroup, B = min(64, ceil(capacity / 256)).  A wave takes one keyframe per step, lane
//     l the words l, l + 64, ... (for M = 512 one 256-byte line per keyframe), eight keyframes in flight; per word
//     popcount((x | x>>1 | x>>2 | x>>3) & 0x11111111) of x = word ^ query word, then a wave reduction by xor-shuffles.  Lane
//     0 keeps the wave's k smallest keys sorted in LDS; the workgroup's waves are merged by a rank sort (keys are distinct
//     but for the all-ones fillers, which tie by position).  B == 1 writes the result; otherwise the B lists go to a
//     stream-ordered scratch allocation and a one-workgroup launch per query merges them the same way.
//   insert: one launch of one workgroup of 1024 lanes that walks the n frames in order - search (as above, 16 waves), decide
//     (one lane), append (all lanes) - with a workgroup barrier between the steps, so a frame sees what the frames before it
//     added.  count is read and written on the device only.
// No float atomics, no workgroup waits for another, the host never waits; every written value is an ordinary vector store.
// The bits are the same on every run, and n frames in one call give the bits of n calls.
#include <cmath>

#include "ojf_common.h"

namespace ojf {

constexpr int kRelocMaxCells = 1024;
constexpr int kRelocMaxFerns = 4096;
constexpr int kRelocMaxWords = kRelocMaxFerns / 8;  // 512
constexpr int kRelocMaxK = 16;
constexpr int kEncodeBlock = 1024;
constexpr int kQueryWaves = 16;
constexpr int kQueryBlock = 64 * kQueryWaves;
constexpr int kQueryMaxBlocks = 64;
constexpr int kQueryBatch = 8;  // keyframes a wave keeps in flight
constexpr int kInsertBlock = 1024;
constexpr int kInsertWaves = kInsertBlock / 64;
constexpr unsigned long long kNoKey = ~0ull;

struct EncodeLaunch {
    const float *depth;
    const uint8_t *mask;     // or NULL
    const uint32_t *image;   // one u32 per pixel, or NULL
    const int32_t *fern_cell;
    const uint8_t *fern_channel;
    const float *fern_threshold;
    uint32_t *codes;
    float *code_image;       // or NULL
    int h, w, cell, CH, CW, n_ferns, vec4;
};

__device__ __forceinline__ bool reloc_quantise(float d, uint32_t &q)
{
    const bool v = fabsf(d) < INFINITY && d > 0.0f && d < 64.0f;
    q = v ? (uint32_t)rintf(d * 1024.0f) : 0u;
    return v;
}

__global__ __launch_bounds__(kEncodeBlock) void reloc_encode_kernel(EncodeLaunch L)
{
    __shared__ unsigned long long s_depth[kRelocMaxCells];  // n << 32 | S
    __shared__ unsigned long long s_color[kRelocMaxCells];  // R | G << 21 | B << 42
    __shared__ float s_val[4][kRelocMaxCells];
    __shared__ uint8_t s_valid[kRelocMaxCells];

    const int tid = threadIdx.x;
    const int c = L.cell, CH = L.CH, CW = L.CW, cells = CH * CW;
    const size_t px0 = (size_t)blockIdx.x * (size_t)L.h * (size_t)L.w;
    const float *depth = L.depth + px0;
    const uint8_t *mask = L.mask ? L.mask + px0 : nullptr;
    const uint32_t *image = L.image ? L.image + px0 : nullptr;

    for (int i = tid; i < cells; i += kEncodeBlock) {
        s_depth[i] = 0ull;
        s_color[i] = 0ull;
    }
    __syncthreads();

    const int rows = CH * c, cols = CW * c;
    if (L.vec4) {
        const int qw = cols >> 2, total = rows * qw;
#pragma unroll 4
        for (int t = tid; t < total; t += kEncodeBlock) {
            const int r = t / qw, x = (t - r * qw) << 2;
            const size_t at = (size_t)r * L.w + x;
            const int ci = (r / c) * CW + x / c;
            const float4 d4 = *reinterpret_cast<const float4 *>(depth + at);
            uint32_t m4 = 0x01010101u;
            if (mask) m4 = *reinterpret_cast<const uint32_t *>(mask + at);
            const float d[4] = {d4.x, d4.y, d4.z, d4.w};
            unsigned long long add = 0ull;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t q;
                const bool v = reloc_quantise(d[e], q) && ((m4 >> (8 * e)) & 0xffu) != 0u;
                if (v) add += (1ull << 32) | q;
            }
            if (add) atomicAdd(&s_depth[ci], add);
            if (image) {
                const uint4 p4 = *reinterpret_cast<const uint4 *>(image + at);
                const uint32_t p[4] = {p4.x, p4.y, p4.z, p4.w};
                unsigned long long rgb = 0ull;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    rgb += (unsigned long long)(p[e] & 0xffu) | (unsigned long long)((p[e] >> 8) & 0xffu) << 21 |
                           (unsigned long long)((p[e] >> 16) & 0xffu) << 42;
                atomicAdd(&s_color[ci], rgb);
            }
        }
    } else {
        const int total = rows * cols;
        for (int t = tid; t < total; t += kEncodeBlock) {
            const int r = t / cols, x = t - r * cols;
            const size_t at = (size_t)r * L.w + x;
            const int ci = (r / c) * CW + x / c;
            uint32_t q;
            const bool v = reloc_quantise(depth[at], q) && (!mask || mask[at] != 0);
            if (v) atomicAdd(&s_depth[ci], (1ull << 32) | q);
            if (image) {
                const uint32_t p = image[at];
                atomicAdd(&s_color[ci], (unsigned long long)(p & 0xffu) | (unsigned long long)((p >> 8) & 0xffu) << 21 |
                                            (unsigned long long)((p >> 16) & 0xffu) << 42);
            }
        }
    }
    __syncthreads();

    // the code image
    const float area = (float)(c * c);
    for (int i = tid; i < cells; i += kEncodeBlock) {
        const unsigned long long a = s_depth[i], b = s_color[i];
        const uint32_t S = (uint32_t)a, n = (uint32_t)(a >> 32);
        const bool valid = 2u * n >= (uint32_t)(c * c);
        const float v0 = valid ? ((float)S / (float)n) * 0.0009765625f : 0.0f;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (image) {
            v[0] = (float)(uint32_t)(b & 0x1fffffu) / area;
            v[1] = (float)(uint32_t)((b >> 21) & 0x1fffffu) / area;
            v[2] = (float)(uint32_t)((b >> 42) & 0x1fffffu) / area;
        }
        s_valid[i] = valid;
        s_val[0][i] = v0; s_val[1][i] = v[0]; s_val[2][i] = v[1]; s_val[3][i] = v[2];
        if (L.code_image) {
            float *o = L.code_image + (size_t)blockIdx.x * 4 * cells + i;
            o[0] = v0; o[cells] = v[0]; o[2 * (size_t)cells] = v[1]; o[3 * (size_t)cells] = v[2];
        }
    }
    __syncthreads();

    // the ferns: one per lane, eight neighbouring lanes make a word (every lane of a wave stays in the loop for the shuffles)
    const int M = L.n_ferns;
    uint32_t *codes = L.codes + (size_t)blockIdx.x * (M >> 3);
    for (int base = 0; base < M; base += kEncodeBlock) {
        const int m = base + tid;
        uint32_t word = 0u;
        if (m < M) {
            const int4 fc = reinterpret_cast<const int4 *>(L.fern_cell)[m];
            const uint32_t ch4 = reinterpret_cast<const uint32_t *>(L.fern_channel)[m];
            const float4 th = reinterpret_cast<const float4 *>(L.fern_threshold)[m];
            const int cell_j[4] = {fc.x, fc.y, fc.z, fc.w};
            const float thr_j[4] = {th.x, th.y, th.z, th.w};
            uint32_t nib = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ci = cell_j[j];
                const int ch = (ch4 >> (8 * j)) & 3u;
                bool bit = false;
                if (ci >= 0 && ci < cells) bit = s_val[ch][ci] > thr_j[j] && (ch != 0 || s_valid[ci] != 0);
                nib |= (uint32_t)bit << j;
            }
            word = nib << (4 * (m & 7));
        }
        word |= __shfl_xor(word, 1);
        word |= __shfl_xor(word, 2);
        word |= __shfl_xor(word, 4);
        if (m < M && (m & 7) == 0) codes[m >> 3] = word;
    }
}

// ---- dissimilarity -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t nibbles_differ(uint32_t x)
{
    return __popc((x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// total[b] = the number of ferns in which keyframe i0 + b * stride differs from the query in s_q (LDS), for the keyframes of
// those below `count`, to every lane of the wave: lane l takes the words l, l + 64, ..., and the loads of all kQueryBatch
// keyframes are issued before the first sum is reduced.  i0, stride and count are uniform over the wave.
__device__ __forceinline__ void wave_differ_batch(const uint32_t *db_codes, const uint32_t *s_q, int W, int i0, int stride, int count,
                                                  int lane, uint32_t total[kQueryBatch])
{
#pragma unroll
    for (int b = 0; b < kQueryBatch; ++b) {
        const int i = i0 + b * stride;
        total[b] = 0u;
        if (i < count) {
            const uint32_t *row = db_codes + (size_t)i * W;
            for (int j = lane; j < W; j += 64) total[b] += nibbles_differ(row[j] ^ s_q[j]);
        }
    }
#pragma unroll
    for (int b = 0; b < kQueryBatch; ++b) total[b] = wave_sum(total[b]);
}

// Lane 0's sorted list of the k smallest keys: `list` is the wave's own k entries.
__device__ __forceinline__ void keep_smallest(unsigned long long *list, int k, unsigned long long key)
{
    if (key >= list[k - 1]) return;
    int p = k - 1;
    while (p > 0 && list[p - 1] > key) {
        list[p] = list[p - 1];
        --p;
    }
    list[p] = key;
}

// out[0..k) = the k smallest of keys[0..count) ascending, ties by position; called by every lane of the workgroup after a
// barrier behind the writes of `keys` (LDS).  count >= k.
__device__ __forceinline__ void rank_select(const unsigned long long *keys, int count, int k, unsigned long long *out)
{
    for (int t = threadIdx.x; t < count; t += blockDim.x) {
        const unsigned long long key = keys[t];
        int rank = 0;
        for (int o = 0; o < count; ++o) {
            const unsigned long long other = keys[o];
            rank += (other < key) | ((other == key) & (o < t));
        }
        if (rank < k) out[rank] = key;
    }
}

__device__ __forceinline__ int store_count(const int32_t *db_count, int capacity)
{
    const int c = *db_count;
    return c < 0 ? 0 : (c > capacity ? capacity : c);
}

// grid (B, n).  out: keys [n][k] when gridDim.x == 1, else the scratch [n][B][k].
__global__ __launch_bounds__(kQueryBlock) void reloc_query_kernel(const uint32_t *codes, int W, const uint32_t *db_codes,
                                                                  const int32_t *db_count, int capacity, int k,
                                                                  unsigned long long *out)
{
    __shared__ uint32_t s_q[kRelocMaxWords];
    __shared__ unsigned long long s_list[kQueryWaves * kRelocMaxK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t *q = codes + (size_t)blockIdx.y * W;
    for (int j = tid; j < W; j += kQueryBlock) s_q[j] = q[j];
    for (int j = tid; j < kQueryWaves * kRelocMaxK; j += kQueryBlock) s_list[j] = kNoKey;
    __syncthreads();

    const int count = store_count(db_count, capacity);
    unsigned long long *list = s_list + wave * k;
    const int stride = gridDim.x * kQueryWaves;
    for (int i0 = blockIdx.x * kQueryWaves + wave; i0 < count; i0 += kQueryBatch * stride) {
        uint32_t total[kQueryBatch];
        wave_differ_batch(db_codes, s_q, W, i0, stride, count, lane, total);
#pragma unroll
        for (int b = 0; b < kQueryBatch; ++b) {
            const int i = i0 + b * stride;
            if (lane == 0 && i < count) keep_smallest(list, k, (unsigned long long)total[b] << 32 | (uint32_t)i);
        }
    }
    __syncthreads();
    unsigned long long *dst = out + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * k;
    rank_select(s_list, kQueryWaves * k, k, dst);
}

// grid (n): the k smallest of the B lists of a query
__global__ __launch_bounds__(kQueryMaxBlocks * kRelocMaxK) void reloc_merge_kernel(const unsigned long long *partial, int B, int k,
                                                                                  unsigned long long *keys)
{
    __shared__ unsigned long long s_keys[kQueryMaxBlocks * kRelocMaxK];
    const int count = B * k;
    for (int t = threadIdx.x; t < count; t += blockDim.x) s_keys[t] = partial[(size_t)blockIdx.x * count + t];
    __syncthreads();
    rank_select(s_keys, count, k, keys + (size_t)blockIdx.x * k);
}

struct InsertLaunch {
    const uint32_t *codes;
    const double *poses;
    uint32_t *db_codes;
    double *db_poses;
    int32_t *db_count;
    unsigned long long *best;
    int32_t *added;
    int n, W, min_differ, force, capacity;
};

__global__ __launch_bounds__(kInsertBlock) void reloc_insert_kernel(InsertLaunch L)
{
    __shared__ uint32_t s_q[kRelocMaxWords];
    __shared__ unsigned long long s_min[kInsertWaves];
    __shared__ int s_count, s_slot;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = L.W;
    if (tid == 0) s_count = store_count(L.db_count, L.capacity);
    for (int f = 0; f < L.n; ++f) {
        const uint32_t *q = L.codes + (size_t)f * W;
        __syncthreads();  // s_count, and the rows the frame before added, are written; s_q and s_min are free
        for (int j = tid; j < W; j += kInsertBlock) s_q[j] = q[j];
        __syncthreads();
        const int count = s_count;
        unsigned long long best = kNoKey;
        for (int i0 = wave; i0 < count; i0 += kQueryBatch * kInsertWaves) {
            uint32_t total[kQueryBatch];
            wave_differ_batch(L.db_codes, s_q, W, i0, kInsertWaves, count, lane, total);
#pragma unroll
            for (int b = 0; b < kQueryBatch; ++b) {
                const unsigned long long key = (unsigned long long)total[b] << 32 | (uint32_t)(i0 + b * kInsertWaves);
                best = i0 + b * kInsertWaves < count && key < best ? key : best;
            }
        }
        if (lane == 0) s_min[wave] = best;
        __syncthreads();
        if (tid == 0) {
            best = kNoKey;
            for (int v = 0; v < kInsertWaves; ++v) best = s_min[v] < best ? s_min[v] : best;
            const bool wanted = L.force || count == 0 || (int)(best >> 32) > L.min_differ;
            const int flag = !wanted ? 0 : (count == L.capacity ? 2 : 1);
            L.best[f] = best;
            L.added[f] = flag;
            s_slot = flag == 1 ? count : -1;
            if (flag == 1) s_count = count + 1;
        }
        __syncthreads();
        const int slot = s_slot;
        if (slot >= 0) {
            uint32_t *row = L.db_codes + (size_t)slot * W;
            for (int j = tid; j < W; j += kInsertBlock) row[j] = s_q[j];
            if (tid < 12) L.db_poses[(size_t)slot * 12 + tid] = L.poses[(size_t)f * 12 + tid];
        }
    }
    __syncthreads();
    if (tid == 0) *L.db_count = s_count;
}

static bool reloc_ferns_ok(int n_ferns) { return n_ferns >= 8 && n_ferns <= kRelocMaxFerns && (n_ferns & 7) == 0; }

}  // namespace ojf

OJF_API int ojf_reloc_encode(const float *depth, const uint8_t *mask, const uint8_t *image, int n, int h, int w, int cell,
                             int n_ferns, const int32_t *fern_cell, const uint8_t *fern_channel, const float *fern_threshold,
                             uint32_t *codes, float *code_image, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_reloc_encode";
    if (!depth || !fern_cell || !fern_channel || !fern_threshold || !codes) return refuse(who, "null pointer argument");
    if (n < 1 || h < 1 || w < 1) return refuse(who, "n, h and w must be >= 1");
    if ((int64_t)n * h * w > 0x7fffffffLL) return refuse(who, "images too large");
    if (cell < 1 || cell > 64) return refuse(who, "cell must be 1..64");
    const int CH = h / cell, CW = w / cell;
    if (CH < 1 || CW < 1) return refuse(who, "cell larger than the frame");
    if ((int64_t)CH * CW > kRelocMaxCells) return refuse(who, "more than 1024 cells: choose a larger cell");
    if (!reloc_ferns_ok(n_ferns)) return refuse(who, "n_ferns must be a multiple of 8 in 8..4096");
    if (((uintptr_t)depth & 3) || ((uintptr_t)image & 3) || ((uintptr_t)codes & 3) || ((uintptr_t)code_image & 3) ||
        ((uintptr_t)fern_channel & 3))
        return refuse(who, "depth_dev, image_dev, codes_dev, code_image_dev and fern_channel_dev must be 4-byte aligned");
    if (((uintptr_t)fern_cell & 15) || ((uintptr_t)fern_threshold & 15))
        return refuse(who, "fern_cell_dev and fern_threshold_dev must be 16-byte aligned");

    EncodeLaunch L;
    L.depth = depth; L.mask = mask; L.image = reinterpret_cast<const uint32_t *>(image);
    L.fern_cell = fern_cell; L.fern_channel = fern_channel; L.fern_threshold = fern_threshold;
    L.codes = codes; L.code_image = code_image;
    L.h = h; L.w = w; L.cell = cell; L.CH = CH; L.CW = CW; L.n_ferns = n_ferns;
    L.vec4 = (w & 3) == 0 && (cell & 3) == 0 && ((uintptr_t)depth & 15) == 0 && ((uintptr_t)mask & 3) == 0 &&
             ((uintptr_t)image & 15) == 0;
    hipLaunchKernelGGL(reloc_encode_kernel, dim3(n), dim3(kEncodeBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_reloc_query(const uint32_t *codes, int n, int n_ferns, const uint32_t *db_codes, const int32_t *db_count,
                            int capacity, int k, uint64_t *keys, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_reloc_query";
    if (!codes || !db_codes || !db_count || !keys) return refuse(who, "null pointer argument");
    if (n < 1 || n > 65535) return refuse(who, "n must be 1..65535");
    if (!reloc_ferns_ok(n_ferns)) return refuse(who, "n_ferns must be a multiple of 8 in 8..4096");
    if (capacity < 1 || capacity > (1 << 24)) return refuse(who, "capacity must be 1..2^24");
    if (k < 1 || k > kRelocMaxK) return refuse(who, "k must be 1..16");
    if (((uintptr_t)codes & 3) || ((uintptr_t)db_codes & 3) || ((uintptr_t)db_count & 3) || ((uintptr_t)keys & 7))
        return refuse(who, "codes_dev, db_codes_dev and db_count_dev must be 4-byte and keys_dev 8-byte aligned");

    const int W = n_ferns / 8;
    int B = (capacity + 255) / 256;
    if (B > kQueryMaxBlocks) B = kQueryMaxBlocks;
    hipStream_t st = as_stream(stream);
    unsigned long long *out = reinterpret_cast<unsigned long long *>(keys);
    if (B == 1) {
        hipLaunchKernelGGL(reloc_query_kernel, dim3(1, n), dim3(kQueryBlock), 0, st, codes, W, db_codes, db_count, capacity, k, out);
        OJF_HIP(hipGetLastError());
        return 0;
    }
    void *scratch = nullptr;  // stream-ordered: the host never waits and calls on other streams have their own
    OJF_HIP(hipMallocAsync(&scratch, (size_t)n * B * k * sizeof(unsigned long long), st));
    unsigned long long *partial = static_cast<unsigned long long *>(scratch);
    hipLaunchKernelGGL(reloc_query_kernel, dim3(B, n), dim3(kQueryBlock), 0, st, codes, W, db_codes, db_count, capacity, k, partial);
    int rc = check_hip(hipGetLastError(), "reloc_query_kernel");
    if (!rc) {
        hipLaunchKernelGGL(reloc_merge_kernel, dim3(n), dim3(kQueryMaxBlocks * kRelocMaxK), 0, st, partial, B, k, out);
        rc = check_hip(hipGetLastError(), "reloc_merge_kernel");
    }
    const int rc_free = check_hip(hipFreeAsync(scratch, st), "hipFreeAsync");
    return rc ? rc : rc_free;
}

OJF_API int ojf_reloc_insert(const uint32_t *codes, const double *poses, int n, int n_ferns, int min_differ, int force,
                             uint32_t *db_codes, double *db_poses, int32_t *db_count, int capacity, uint64_t *best,
                             int32_t *added, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_reloc_insert";
    if (!codes || !poses || !db_codes || !db_poses || !db_count || !best || !added) return refuse(who, "null pointer argument");
    if (n < 1) return refuse(who, "n must be >= 1");
    if (!reloc_ferns_ok(n_ferns)) return refuse(who, "n_ferns must be a multiple of 8 in 8..4096");
    if (capacity < 1 || capacity > (1 << 24)) return refuse(who, "capacity must be 1..2^24");
    if (min_differ < 0 || min_differ > n_ferns) return refuse(who, "min_differ must be 0..n_ferns");
    if (((uintptr_t)codes & 3) || ((uintptr_t)db_codes & 3) || ((uintptr_t)db_count & 3) || ((uintptr_t)added & 3) ||
        ((uintptr_t)poses & 7) || ((uintptr_t)db_poses & 7) || ((uintptr_t)best & 7))
        return refuse(who, "the u32 / i32 arrays must be 4-byte, the f64 / u64 arrays 8-byte aligned");

    InsertLaunch L;
    L.codes = codes; L.poses = poses; L.db_codes = db_codes; L.db_poses = db_poses; L.db_count = db_count;
    L.best = reinterpret_cast<unsigned long long *>(best); L.added = added;
    L.n = n; L.W = n_ferns / 8; L.min_differ = min_differ; L.force = force != 0; L.capacity = capacity;
    hipLaunchKernelGGL(reloc_insert_kernel, dim3(1), dim3(kInsertBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    return 0;
}
