// The small pieces the volume and mesh operators (ojf_volume.hip, ojf_mesh*.hip, ojf_raster.hip, ojf_components.hip,
// ojf_distance.hip, ojf_simplify.hip, ojf_resample.hip and the projective sweeps through ojf_projview.h) share, each
// defined once: the one-block prefix sum, the grid of a streaming launch, 3-vector arithmetic, the lanes of packed fp16 /
// u8 registers, the "observed voxel" rule and the host checks of an [X,Y,Z] box.
#pragma once
#include "ojf_common.h"

#include <math.h>
#include <cmath>

namespace ojf {

// ---- one-block exclusive prefix sum ----------------------------------------------------------------------------------
constexpr int kScanBlock = 1024;  // lanes of the block that runs block_exclusive_scan

struct ScanIdentity {
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const { return v; }
};

// out[i] = value(in[0]) + ... + value(in[i-1]) for i in [0, n), in == out allowed; returns the total to every lane (0 for
// n == 0).  For ONE block of kScanBlock lanes, all of which call it: lane t sums its contiguous chunk of ceil(n / 1024)
// values, the chunks' sums are scanned in LDS (Hillis-Steele), lane t writes its chunk's offsets.  Sums are kept in `Sum`
// (uint32_t or unsigned long long) and stored truncated to 32 bits: with 64-bit sums a caller sees from the total whether
// the offsets wrapped.  Indices are 64-bit: no n < 2^32 overflows them.
template <typename Sum, typename Value = ScanIdentity>
__device__ __forceinline__ Sum block_exclusive_scan(const uint32_t *in, uint32_t *out, uint32_t n, Value value = Value())
{
    __shared__ Sum part[kScanBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = n / kScanBlock + (n % kScanBlock ? 1u : 0u);
    const uint64_t first = (uint64_t)t * chunk;
    const uint64_t lo = first < n ? first : n, hi = lo + chunk < n ? lo + chunk : n;
    Sum sum = 0;
    for (uint64_t i = lo; i < hi; ++i) sum += value(in[i]);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
        const Sum add = (int)t >= d ? part[t - d] : (Sum)0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    Sum run = part[t] - sum;
    for (uint64_t i = lo; i < hi; ++i) {
        const uint32_t c = value(in[i]);
        out[i] = (uint32_t)run;
        run += c;
    }
    return part[kScanBlock - 1];
}

// ---- streaming launches ----------------------------------------------------------------------------------------------
static inline int stream_grid(size_t work_items, int block = 256)
{
    size_t blocks = (work_items + block - 1) / block;
    if (blocks > 2048) blocks = 2048;  // 256 CUs x 8 resident blocks, grid-stride the rest
    return blocks ? (int)blocks : 1;
}

// ---- 3-vectors: the operation order is part of the operators' definitions (-ffp-contract=off) ---------------------------
__device__ __forceinline__ float dot3(const float u[3], const float v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ __forceinline__ void cross3(const float u[3], const float v[3], float o[3])
{
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}

__device__ __forceinline__ bool finite3(const float p[3]) { return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY; }

// ---- packed lanes ----------------------------------------------------------------------------------------------------
// element e of 16-bit / 8-bit values packed into 32-bit registers; e is a constant after unrolling
__device__ __forceinline__ uint32_t get16(const uint32_t *q, int e) { return (q[e >> 1] >> ((e & 1) * 16)) & 0xffffu; }
__device__ __forceinline__ void set16(uint32_t *q, int e, uint32_t v)
{
    const int sh = (e & 1) * 16;
    q[e >> 1] = (q[e >> 1] & ~(0xffffu << sh)) | (v << sh);
}

__device__ __forceinline__ uint32_t get8(const uint32_t *q, int e) { return (q[e >> 2] >> ((e & 3) * 8)) & 0xffu; }
__device__ __forceinline__ void set8(uint32_t *q, int e, uint32_t v)
{
    const int sh = (e & 3) * 8;
    q[e >> 2] = (q[e >> 2] & ~(0xffu << sh)) | (v << sh);
}

// the 8 halves of 16-byte group `group` of p (p 16-byte aligned) in one access
__device__ __forceinline__ void load8(const uint16_t *p, size_t group, uint32_t q[4])
{
    const uint4 v = reinterpret_cast<const uint4 *>(p)[group];
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
}

// ---- volumes ---------------------------------------------------------------------------------------------------------
// A voxel of a fused volume counts as observed when its weight is positive and its TSDF is a number (fp16 bit patterns).
__device__ __forceinline__ bool voxel_observed(uint16_t t, uint16_t w)
{
    const float tv = h2f(t);
    return h2f(w) > 0.0f && tv == tv;
}

// ---- host ------------------------------------------------------------------------------------------------------------
static inline bool all_finite(const double *p, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// positive sizes and a voxel count a 31-bit index reaches (sizes that were ints: neither product overflows)
static inline bool volume_size_ok(int64_t X, int64_t Y, int64_t Z)
{
    const int64_t lim = 0x7fffffffLL;
    return X > 0 && Y > 0 && Z > 0 && X * Y <= lim && X * Y * Z <= lim;
}

// What every entry point asks of an [X,Y,Z] box: volume_size_ok; 0 or refuse(who, ...).
static inline int check_volume_size(const char *who, int X, int Y, int Z)
{
    if (X <= 0 || Y <= 0 || Z <= 0) return refuse(who, "non-positive volume size");
    if (!volume_size_ok(X, Y, Z)) return refuse(who, "volume too large");
    return 0;
}

}  // namespace ojf
