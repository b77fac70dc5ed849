// The seam between the fusion net's two halves: what the inference net (ojf_net.hip) and the training path (ojf_train.hip)
// both use, and nothing else.  The training path describes every convolution as ConvArgs and hands it to launch_conv_args;
// that function and every kernel it can launch (conv_mfma_kernel, conv_mfma_lds_kernel, conv_f16x3_kernel,
// conv_f16x3_rows_kernel) are compiled in ojf_net.hip alone, and so is the launch log a launch is counted in.
#pragma once
#include "ojf_common.h"

namespace ojf {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// x (8 fp32 values) -> fp16 halves xh + xl, both rounded to nearest; x - xh is exact in fp32
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void split_f16(const f32x4 &a, const f32x4 &b, f16x8 &hi, f16x8 &lo)
{
    const f32x8 x = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    hi = __builtin_convertvector(x, f16x8);  // 4 x v_cvt_pk_f16_f32
    const u32x4 h = __builtin_bit_cast(u32x4, hi);
    u32x4 l;
#pragma unroll
    for (int i = 0; i < 4; ++i) l[i] = split_lo_pair(h[i], x[2 * i], x[2 * i + 1]);
    lo = __builtin_bit_cast(f16x8, l);
}

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

static inline f32x4 *planes(float *p) { return reinterpret_cast<f32x4 *>(p); }
static inline const f32x4 *planes(const float *p) { return reinterpret_cast<const f32x4 *>(p); }

struct ConvArgs {
    const f32x4 *in;   // input planes (in[-1] is a zero float4); group cg of the window = plane in_g0 + cg
    f32x4 *out;        // output planes (NULL when out_rows is used)
    float *out_rows;   // last layer only: row-major [npix, rows_stride] scalars, channels < rows_n
    const f32x4 *wp;   // packed weights [oc tile][superstep][lane] float4
    const float *bias; // [n_ot*16]
    const float *rinv; // split-fp16: [n_ot*16] inverse of the per-output-channel power-of-two weight scale
    int in_g0, out_g0, rows_stride, rows_n;
    int h, w, npix;
    int taps, dil;
    int c4;          // input channel groups per tap
    int nsteps;      // supersteps = ceil(taps * c4 / 4)
    int og_store;    // output channel groups written (planar mode)
    int act, act_n;  // activation applied to output channels < act_n
    float scale;
    int *ovf;        // split-fp16 only: set to 1 when an activation leaves the fp16 range (host-mapped flag)
    int accum;       // planar stores only: out += result (fan-out gradients of the training path); 0 = plain store
    const float *dscale;  // training backward-data: the input carries a power-of-two factor *dscale - the result is divided by it; NULL = off
    unsigned w_magic, c4_magic;  // ceil(2^32 / w), ceil(2^32 / c4): x / d == umulhi(x, magic) while x * d < 2^32 (0: divide)
    int in_split = 0, out_split = 0;  // split-fp16 launches: the input / output planes are split planes (split_pack4)
    // Banded split-fp16 3x3 launches with dilation r > 1 (round 6): the rows of the image are handed to the blocks in the order
    // (y mod r, y div r) instead of y.  An XCD's band of 30 rows of a 240-row frame then holds rows that are r apart - the
    // very rows its taps read - instead of 30 neighbours whose taps reach 27 rows into both neighbouring bands: with plain
    // bands every private L2 pulled (30 + 2 r) / 30 of its share through the fabric (2.8x for r = 27, 1.6x for r = 9: the
    // grouped launch fetched 40 MB for a 24.6-MB input, profiles/r05_final_traffic_pmc.txt); in class order the halo is one
    // row on either side of the band.  Which block computes which pixels changes, nothing else: the same bits.
    int row_perm = 0, perm_q = 0, perm_rem = 0;  // r (0: off), h / r, h % r
    const f32x4 *wp_rows = nullptr;  // the layer's weights in tap-row order (conv_f16x3_rows_kernel), NULL: not packed for it
};

__device__ __forceinline__ int fast_div(int x, int d, unsigned magic) { return magic ? (int)__umulhi((unsigned)x, magic) : x / d; }

// Split-fp16 range guard.  Kernels keep a running maximum of the magnitudes of every value a later layer will
// split (2 VALU per float4: v_max3_f32 with |.| modifiers) and raise the flag if it exceeds the fp16 range.
// v_max ignores NaN operands, deliberately: a NaN input (the reference writes NaN TSDF into voxels it touches with
// zero total weight, and later frames gather them) propagates to NaN outputs in both arithmetics exactly as in the
// fp32 reference, so it is not an error here either.  With finite weights (checked at creation) an out-of-range
// event is always a finite value beyond 65504 or an infinity at a guarded point first.
__device__ __forceinline__ float guard_max(float mx, const f32x4 &v)
{
    return fmaxf(fmaxf(fmaxf(mx, fabsf(v[0])), fmaxf(fabsf(v[1]), fabsf(v[2]))), fabsf(v[3]));
}

// packed weights: the layouts both halves pack (finish() on the host, train_pack*_kernel on the device)
constexpr int kMaxSteps = 128;  // supersteps per conv (K <= 2048)
constexpr int kPadSteps = 4;    // dead supersteps appended for the three-stage prefetch (fetches reach S+4)
constexpr int kPad16 = 6;  // dead supersteps behind the weights and the tap table (chunk copies + prefetch)
constexpr int kNT = 2;  // packed weights are padded to a multiple of this many output-channel tiles

// (ojf_net.hip)
// Launches n (<= 4) independent convolutions with the same number of output tiles as ONE grid
// (blockIdx.y = problem): the four branches of a VortexPooling run together instead of as four
// under-filled launches with their own ramp-up and tail.
int launch_conv_args(const ConvArgs *args, int n, int nt, hipStream_t st, int arith);
// magic of fast_div for divisor d and dividends below `limit` (0 = use a real division)
unsigned div_magic(int d, uint64_t limit);
// Fork / join events between streams of the same device: no timing and no system-scope fence - nothing here is read by
// the host or another device through these events.
unsigned event_flags();

}  // namespace ojf
