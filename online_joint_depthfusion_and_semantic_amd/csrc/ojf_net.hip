// FUSION NET: eval-mode FusionNet_v3 / FusionNet_v2 (modules/model.py:164-283) as a chain of fused
// convolution kernels on the gfx950 matrix cores.
//
// Arithmetic (ojf_net_set_arithmetic, captured per net at creation), both with fp32 accumulation and
// fp32 activations in memory; tsdf_est agrees with the reference's fp32 CPU net to a few 1e-6
// (tolerance stated in the tests: 1e-5).  The +-0.1 truncation band of the TSDF rules out plain
// bf16/fp16 operands.
//   OJF_ARITH_F32   v_mfma_f32_16x16x4_f32: bitwise a k-ordered fmaf chain; 1024 MAC per 32 cycles.
//   OJF_ARITH_F16X3 (default) split-fp16: x = xh + xl, w = wh + wl with fp16 halves (round to nearest);
//                   x*w ~= wl*xh + wh*xl + wh*xh on v_mfma_f32_16x16x32_f16 (8192 MAC per 16 cycles,
//                   three of them per product block: 5.3x the fp32-input MFMA rate).  The dropped wl*xl
//                   term is <= 2^-22 |x w|; measured layer error is below the fp32 chain's
//                   (tests/microbench/conv_f16x3_bench.hip).  Weight rows are equilibrated by powers of two
//                   (row_scale) so that BN-folded rows of any magnitude keep their mantissa.  Operands must
//                   stay below 65504 in magnitude (fp16 range) - true for TSDF values, fp16 volume weights,
//                   metric depth and the BN-folded activations of a trained net; every kernel guards it
//                   (guard_max, ojf_net_check) and OJF_ARITH_F32 has no such limit.
//
// Data layout ("C4 planes"): an activation tensor with C channels (padded to a multiple of 4:
// 19 -> 20, 114 -> 116; pad channels carry zeros) is stored as C/4 planes of float4, element
// (channel group cg, pixel p) at plane[cg * npix + p].  A wave's 16 consecutive pixels of one
// channel group are 256 contiguous bytes, so every MFMA operand fetch and every result store is a
// fully coalesced 16-byte-per-lane access WITHOUT an LDS transpose (the first version used NHWC rows:
// its fragment-shaped loads touched 64 different cache lines per wave instruction and the kernel
// sat at the texture-addresser limit, ~4x off the MFMA bound).
//
// A convolution is an implicit GEMM  D[oc, pixel] = sum_K W[oc, K] * X[K, pixel]:
//   MFMA rows = 16 output channels (A operand = packed weights), MFMA cols = 16 consecutive pixels
//   (B operand = activations), K = flattened list of (tap, 4-channel group) pairs, G = tap*c4 + cg.
//   fp32: in superstep S lane group g (= lane >> 4) owns group G = 4S + g: it fetches that group's float4 of
//   ITS tap's source pixel and feeds element j to MFMA j of the superstep; split-fp16: a superstep is one
//   32-wide K block, lane group g owns groups 8S + 2g and 8S + 2g + 1, splits its 8 values into fp16 halves
//   and issues 3 MFMAs per output tile.  The packed weights use the same (g, j) permutation.  Any channel count
//   that is a multiple of 4 works without tails, out-of-image taps contribute zeros, supersteps whose every
//   source pixel is outside the image are skipped (dilation 9 / 27 near the borders), and the loop is software
//   pipelined (three operand stages in flight).
//   The accumulator of lane (pixel i, g) holds output channels 4g..4g+3 of its pixel: the epilogue
//   adds bias, applies the activation and writes ONE float4 into the output plane.
//
// Algebraic restructuring of VortexPooling (model.py:100-161), exact up to fp32 rounding:
//   * the four branch-entry 1x1 convolutions commute with the (linear) 3x3 average pools, so they
//     run as ONE 1x1 GEMM on x with 4*mid output channels, and the pools run on mid (19) channels
//     instead of in_chs (114/228);
//   * the global-average branch is constant over the image: it is reduced to a per-frame bias of
//     the final 1x1 convolution (two tiny kernels on a side stream), removing its 114 input columns from that GEMM.
// Launches of one forward pass: decided ONCE, from the net's shape alone, by plan_forward in ojf_net_create (a ForwardPlan: the
// dense stage, one VortexStep per VortexPooling, the head); forward_launches / run_vortex / run_dense only execute it, and
// ojf_net_plan lists its launches without a device.  The shape predicates the planner uses (entry_tiles, fused_tail_form,
// chain_dense_form, ...) also tell the packing code which forms to pack; a new variant starts there ("the forward plan" below).
// Geometry-only v3, the default topology, frame width a multiple of 8: dense_chain_kernel (all dense Blocks of the head), then per VortexPooling {pool pyramid (+ the global-average
// fold), two grouped launches of the four branches' dilated 3x3, fused tail}: the first VortexPooling's entry GEMM is a launch
// of its own (entry1x1_kernel), its tail runs the second one's entry GEMM, and the last tail runs the 11-layer prediction
// head: 10 launches on one stream.  The two-head (semantic) net runs its second head beside the first on a second stream, each
// head's tail computing its half of the last entry GEMM.  Other inputs take the general paths: dense_pair_kernel per Block
// (w % 8 != 0), generic convolutions (fp32 arithmetic, other growth rates), the general VortexPooling flow with the
// global-average branch on a side stream and an unfused tail / head (topologies without chain-layer forms).
// Environment switches: OJF_NET_GRAPH=1 (opt-in hipGraph replay); OJF_NET_TRACE=1 (one stderr line per launch: net_trace_on);
// test-only, set by tests/test_net_gpu.py: OJF_NO_DENSE_CHAIN=1 (pair kernels instead of the chain kernel).
// Files: this unit is the inference net (kernels, packing, the forward plan, the executor, ojf_net_*) with ojf_net_pair.h
// (dense_pair_kernel) and ojf_net_chain.h (dense_chain_kernel) as its parts.  ojf_net_conv.h is what it shares with the training
// path, a unit of its own (ojf_train.hip): ConvArgs and the helpers around it, and the declarations of launch_conv_args,
// div_magic and event_flags, defined here.  The range guard's state and its entry points
// (ojf_net_check, ojf_guard_*) are ojf_guard.hip; this file only passes overflow_flag() to its kernels.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ojf_net_conv.h"

namespace ojf {

// (vector typedefs, split_f16, ConvArgs, fast_div, guard_max, round_up, planes(), the packing constants: ojf_net_conv.h)

// One float4 -> its split-fp16 form in the same 16 bytes: halfs {h0 h1 h2 h3 | l0 l1 l2 l3}, the very halves split_f16
// makes of these values (same pairs, same instructions).  A producer that stores its planes this way ("split planes")
// spares every consumer tap the split: the grouped 3x3 convolutions re-split each input value nine times, 12 of the
// ~19 VALU instructions a 16-pixel tile costs per superstep.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 split_pack4(const f32x4 &x)
{
    const f16x4 hi = __builtin_convertvector(x, f16x4);  // 2 x v_cvt_pk_f16_f32
    const u32x2 h = __builtin_bit_cast(u32x2, hi);
    const u32x4 r{h[0], h[1], split_lo_pair(h[0], x[0], x[1]), split_lo_pair(h[1], x[2], x[3])};
    return __builtin_bit_cast(f32x4, r);
}
// split planes -> fp32: hi + lo (exact: the halves have 11 + 11 significant bits)
__device__ __forceinline__ f32x4 unsplit4(const f32x4 &s)
{
    typedef _Float16 f16x8_ __attribute__((ext_vector_type(8)));
    const f16x8_ h = __builtin_bit_cast(f16x8_, s);
    return f32x4{(float)h[0] + (float)h[4], (float)h[1] + (float)h[5], (float)h[2] + (float)h[6], (float)h[3] + (float)h[7]};
}
// two split-plane float4 (channel groups A, B) -> the MFMA operand halves of their eight channels:
// (A0 A1 A2 A3)(B0 B1 B2 B3) -> (A0 A1 B0 B1)(A2 A3 B2 B3).
// Plain shuffles on purpose: round 3's two hand-placed v_swap_b32 (inline assembly, which hipcc's hazard recogniser does not look
// into) computed wrong sums next to the MFMAs of dense_chain_kernel and measured no faster (2533 / 2538 against 2539 / 2542 frames/s).
__device__ __forceinline__ void unpack_split(const f32x4 &a, const f32x4 &b, f16x8 &hi, f16x8 &lo)
{
    hi = __builtin_bit_cast(f16x8, __builtin_shufflevector(a, b, 0, 1, 4, 5));
    lo = __builtin_bit_cast(f16x8, __builtin_shufflevector(a, b, 2, 3, 6, 7));
}

// acc += W * X for one 16x16 tile over a 32-wide K block, W and X given as split halves
__device__ __forceinline__ f32x4 mfma_f16x3(const f32x4 &wh, const f32x4 &wl, const f16x8 &xh, const f16x8 &xl, f32x4 acc)
{
    const f16x8 h = __builtin_bit_cast(f16x8, wh), l = __builtin_bit_cast(f16x8, wl);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(l, xh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(h, xl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(h, xh, acc, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// position `pr` of the row order (y mod r, y div r) -> row y; classes c < h % r have h / r + 1 rows, the others h / r
__device__ __forceinline__ int perm_row(int pr, int r, int q, int rem)
{
    const int big = rem * (q + 1);
    if (pr < big) {
        const int c = pr / (q + 1);
        return c + (pr - c * (q + 1)) * r;
    }
    const int p2 = pr - big, c = p2 / q;
    return rem + c + (p2 - c * q) * r;
}

__device__ __forceinline__ bool beyond_f16(const f32x4 &v)  // raw inputs; NaN is not a range violation (see guard_max)
{
    return guard_max(0.0f, v) > 65504.0f;
}
__device__ __forceinline__ f32x4 fma4(const f32x4 &a, const f32x4 &b, const f32x4 &c)
{
    return f32x4{__builtin_fmaf(a[0], b[0], c[0]), __builtin_fmaf(a[1], b[1], c[1]), __builtin_fmaf(a[2], b[2], c[2]),
                 __builtin_fmaf(a[3], b[3], c[3])};
}

// ReLU / LeakyReLU / identity are one select with a slope (0, 0.01, 1); Tanh is a separate,
// wave-uniform path (last layer only)
__device__ __forceinline__ float act_slope(int act)
{
    return act == OJF_ACT_RELU ? 0.0f : (act == OJF_ACT_LEAKY ? 0.01f : 1.0f);
}
// x > 0 ? x : slope * x for 0 <= slope <= 1 as max(x, slope * x): one multiply (packed with its neighbour) + one max
// instead of compare + select + multiply - a third of the VALU instructions of the fused tails were activations.  The
// same bits for every finite x, +-0 and NaN (max(NaN, NaN) = NaN); -inf under ReLU gives -inf where the select form gave
// NaN (-inf * 0) - both are outside the range the split-fp16 guard admits.
// (v_max_f32 by hand: fmaxf() makes the compiler canonicalise both operands with an extra max each and unpack the
// neighbouring packed multiplies)
__device__ __forceinline__ float leaky_max(float x, float slope)
{
    const float sx = slope * x;
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(sx));
    return r;
}
__device__ __forceinline__ f32x4 leaky_max4(const f32x4 &x, float slope)
{
    const f32x4 sx = x * slope;  // two v_pk_mul_f32
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) asm("v_max_f32 %0, %1, %2" : "=v"(r[j]) : "v"(x[j]), "v"(sx[j]));
    return r;
}


// C/D layout of the 16x16 MFMAs: lane (i16, g) holds column i16 (pixel) and rows 4g..4g+3 (output channels)
template <int MT, int NT, bool GUARD = false>
__device__ __forceinline__ void conv_epilogue(const ConvArgs &a, const f32x4 (&acc)[MT][NT], int strip, int i16, int g,
                                              const f32x4 (&bvec)[NT], const f32x4 (&rvec)[NT])
{
    const float slope = act_slope(a.act);
    const bool use_tanh = a.act == OJF_ACT_TANH;
    const float oscale = a.dscale ? a.scale / *a.dscale : a.scale;
    float gmax = 0.0f;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int og = n * 4 + g;  // output channel group
        const f32x4 b = bvec[n];
        const f32x4 ri = rvec[n];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int p = strip + m * 16 + i16;
            const f32x4 lin4 = GUARD ? fma4(acc[m][n], ri, b) : acc[m][n] + b;
            f32x4 v = lin4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float lin = v[j];
                float r = lin > 0.0f ? lin : lin * slope;
                if (use_tanh) r = tanhf(lin);
                v[j] = (og * 4 + j < a.act_n ? r : lin) * oscale;
            }
            if (p >= a.npix) continue;
            if (a.out_rows) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (og * 4 + j < a.rows_n) a.out_rows[(size_t)p * a.rows_stride + og * 4 + j] = v[j];
            } else if (og < a.og_store) {
                f32x4 *dst = a.out + (size_t)(a.out_g0 + og) * a.npix + p;
                if (a.accum) v += *dst;
                *dst = a.out_split ? split_pack4(v) : v;
                if constexpr (GUARD) gmax = guard_max(gmax, lin4);  // pre-activation magnitude
            }
        }
    }
    if constexpr (GUARD)
        if (gmax > 65504.0f && a.ovf) guard_raise(a.ovf, 1);
}

// The common case of the split-fp16 launches - planar output, ReLU / LeakyReLU / no activation on every stored channel,
// unit scale, plain store - without the generic epilogue's per-value branches (row output, tanh, partial activation,
// scale pointers): the same operations on the same values in the same order, i.e. the same bits, in ~1/3 of the
// instructions (the grouped 19 -> 19 convolutions issue 9 VALU per MFMA and half of a wave's instructions were its
// prologue and epilogue: r03_final_inst_counters.txt).  The host picks it per launch (conv_lean_ok).
// tile0[m]: first pixel of the wave's 16-pixel tile m
template <int MT, int NT>
__device__ __forceinline__ void conv_epilogue_lean(const ConvArgs &a, const f32x4 (&acc)[MT][NT], const int (&tile0)[MT], int i16, int g,
                                                   const f32x4 (&bvec)[NT], const f32x4 (&rvec)[NT])
{
    const float slope = act_slope(a.act);
    float gmax = 0.0f;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int og = n * 4 + g;
        if (og >= a.og_store) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int p = tile0[m] + i16;
            const f32x4 lin4 = fma4(acc[m][n], rvec[n], bvec[n]);
            const f32x4 v = leaky_max4(lin4, slope);
            if (p < a.npix) {
                a.out[(size_t)(a.out_g0 + og) * a.npix + p] = a.out_split ? split_pack4(v) : v;
                gmax = guard_max(gmax, lin4);
            }
        }
    }
    if (gmax > 65504.0f && a.ovf) guard_raise(a.ovf, 1);
}

static inline bool conv_lean_ok(const ConvArgs &a)
{
    return !a.out_rows && a.act != OJF_ACT_TANH && (a.act == OJF_ACT_NONE || a.act_n >= 4 * a.og_store) && a.scale == 1.0f && !a.dscale && !a.accum;
}

// Per-(superstep, slot) source table: float4 index of the tap's plane origin relative to a.in (-1 = the zero
// float4 every activation buffer keeps in front of its planes) and the tap's (dy, dx) packed in one int.
__device__ __forceinline__ void build_tap_table(int2 *tab, const ConvArgs &a, int entries)
{
    for (int G = threadIdx.x; G < entries; G += 256) {
        const int t = G / a.c4, cg = G - t * a.c4;
        int off = -1, dy = -30000, dx = 0;
        if (t < a.taps) {
            dy = dx = 0;
            if (a.taps == 9) {
                const int ky = t / 3;
                dy = (ky - 1) * a.dil;
                dx = (t - 3 * ky - 1) * a.dil;
            }
            off = (a.in_g0 + cg) * a.npix + dy * a.w + dx;
        }
        tab[G] = int2{off, (int)(((unsigned)dy << 16) | ((unsigned)dx & 0xffffu))};
    }
}

// split-fp16 kernel: byte offset of the tap's plane origin relative to a.in, and the tap's bit (0 = dead entry)
__device__ __forceinline__ void build_tap_table16(int2 *tab, const ConvArgs &a, int entries)
{
    for (int G = threadIdx.x; G < entries; G += 256) {
        const int t = fast_div(G, a.c4, a.c4_magic), cg = G - t * a.c4;
        int off = 0, bit = 0;
        if (t < a.taps) {
            int dy = 0, dx = 0;
            if (a.taps == 9) {
                const int ky = t / 3;
                dy = (ky - 1) * a.dil;
                dx = (t - 3 * ky - 1) * a.dil;
            }
            off = ((a.in_g0 + cg) * a.npix + dy * a.w + dx) * 16;
            bit = 1 << t;
        }
        tab[G] = int2{off, bit};
    }
}

// ABL is a profiling-only ablation mask (tests/microbench): 1 = no activation loads, 2 = no weight
// loads, 4 = no MFMA, 8 = no per-superstep index math.  Product launches always use ABL = 0.
struct ConvGroup {
    ConvArgs g[4];  // independent convolutions of identical tile shape run as one launch (blockIdx.y)
    int nblocks;    // XCD-banded launches: pixel blocks of the image (gridDim.x is that rounded up to 8); 0 = plain order
    // PERSISTENT split-fp16 launches (round 6; layers whose whole packed weights are ONE LDS chunk: the grouped 19 -> 19 3x3): a
    // block walks `band` = round_up(nblocks, 8) / 8 logical pixel blocks of ITS XCD's band in steps of gridDim.x / 8 and
    // copies the tap table and the 24 KB of weights ONCE - with one pixel block per launch block every 128 pixels (10 KB of
    // input) paid a 24-KB weight copy, a table build and three barriers, 2400 times per branch and launch.  0 = off.
    int band = 0;
};

// (xcd_band_block / banded_block_x: ojf_common.h)

// SKIP: skip supersteps whose every source pixel lies outside the image (worth it for dilation 9 / 27);
// without it the loop body is one basic block and the scheduler interleaves the next fetch's address
// math with the MFMAs.
template <int MT, int NT, int ABL = 0, bool SKIP = true>
__global__ __launch_bounds__(256) void conv_mfma_kernel(const ConvGroup grp)
{
    const ConvArgs &a = grp.g[blockIdx.y];
    // tap table built once per block; kPadSteps dead supersteps pad the end so that the three-stage
    // prefetch needs no tail handling
    __shared__ int2 tab[(kMaxSteps + kPadSteps) * 4];
    build_tap_table(tab, a, (a.nsteps + kPadSteps) * 4);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int strip = (blockIdx.x * 4 + wave) * (MT * 16);
    if (strip >= a.npix) return;
    constexpr int ot0 = 0;  // a wave covers every output-channel tile

    int py[MT], px[MT], plin[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int p = strip + m * 16 + i16;
        plin[m] = p;
        py[m] = p < a.npix ? p / a.w : -0x40000000;  // rows far outside the image for padding lanes
        px[m] = p - (p / a.w) * a.w;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const f32x4 *wb[NT];  // packed weights carry kPadSteps zero supersteps at the end as well
#pragma unroll
    for (int n = 0; n < NT; ++n) wb[n] = a.wp + (size_t)(ot0 + n) * (a.nsteps + kPadSteps) * 64 + lane;
    // activations through a buffer resource: an invalid tap selects an out-of-range offset, which loads zeros - the
    // input needs no zero float4 in front of its planes (the training path feeds plain torch allocations)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<f32x4 *>(a.in), 0, (a.in_g0 + a.c4) * a.npix * 16, 0x00020000);

    // Operand fetch of superstep S.  Nothing consumes the loaded values before the MFMAs (invalid
    // taps select the INDEX of the zero float4 instead of masking data), so three stages stay in
    // flight behind counted waits.
    auto fetch = [&](f32x4(&xv)[MT], f32x4(&wv)[NT], int S, bool &live) {
        if constexpr (ABL & 8) {
            live = true;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if constexpr (ABL & 1) xv[m] = f32x4{1.f, 2.f, 3.f, 4.f};
                else xv[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)plin[m] * 16u, 0, 0));
            }
        } else {
            const int2 e = tab[S * 4 + g];
            const int dy = e.y >> 16, dx = (int)(short)(e.y & 0xffff);
            bool any_ok = false;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const bool ok = (unsigned)(py[m] + dy) < (unsigned)a.h && (unsigned)(px[m] + dx) < (unsigned)a.w;
                const unsigned boff = ok ? (unsigned)(e.x + plin[m]) * 16u : 0xffffffffu;
                if constexpr (ABL & 1) {
                    xv[m] = f32x4{1.f, 2.f, 3.f, 4.f};
                    asm volatile("" ::"v"(boff));
                } else {
                    xv[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, boff, 0, 0));
                }
                any_ok |= ok;
            }
            live = SKIP ? __any(any_ok) : true;  // dead superstep: every source pixel of the wave is outside the image
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            if constexpr (ABL & 2) wv[n] = f32x4{1.f, 1.f, 1.f, 1.f};
            else wv[n] = wb[n][(size_t)S * 64];
        }
    };
    auto mac = [&](const f32x4(&xv)[MT], const f32x4(&wv)[NT]) {
        if constexpr (ABL & 4) {
#pragma unroll
            for (int m = 0; m < MT; ++m) asm volatile("" ::"v"(xv[m][0]), "v"(xv[m][1]), "v"(xv[m][2]), "v"(xv[m][3]));
#pragma unroll
            for (int n = 0; n < NT; ++n) asm volatile("" ::"v"(wv[n][0]), "v"(wv[n][1]), "v"(wv[n][2]), "v"(wv[n][3]));
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[n][j], xv[m][j], acc[m][n], 0, 0, 0);
    };

    // three operand stages in flight: superstep S+2 is fetched while S computes
    f32x4 x0[MT], w0[NT], x1[MT], w1[NT], x2[MT], w2[NT];
    bool l0, l1, l2;
    fetch(x0, w0, 0, l0);
    fetch(x1, w1, 1, l1);
    for (int S = 0; S < a.nsteps; S += 3) {
        fetch(x2, w2, S + 2, l2);
        if (!SKIP || l0) mac(x0, w0);
        fetch(x0, w0, S + 3, l0);
        if (!SKIP || l1) mac(x1, w1);
        fetch(x1, w1, S + 4, l1);
        if (!SKIP || l2) mac(x2, w2);
    }

    f32x4 bvec[NT], rvec[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        bvec[n] = *reinterpret_cast<const f32x4 *>(a.bias + (size_t)n * 16 + 4 * g);
        rvec[n] = f32x4{1.f, 1.f, 1.f, 1.f};
    }
    conv_epilogue<MT, NT>(a, acc, strip, i16, g, bvec, rvec);
}

// Wide fp32 launches (NT >= 6 output tiles: the training path's 1x1 layers on 114 .. 580 channels and their
// backward-data forms): the weight fragments of a superstep are 1 KB per output tile and every wave of the plain kernel
// fetches all of them for its 16 pixels - 4800 waves x 64 KB through the L1s per launch of the transposed final
// convolution, which ran at 16 % of the fp32-MFMA peak for it.  Here the four waves of a block share one copy of a
// three-superstep chunk in LDS (the split-fp16 kernel's scheme): same arithmetic, same order, same bits.
template <int NT>
__global__ __launch_bounds__(256) void conv_mfma_lds_kernel(const ConvGroup grp)
{
    constexpr int CS = 3;
    const ConvArgs &a = grp.g[blockIdx.y];
    __shared__ int2 tab[(kMaxSteps + kPadSteps) * 4];
    __shared__ f32x4 wl[CS * NT * 64];
    build_tap_table(tab, a, (a.nsteps + kPadSteps) * 4);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int strip = (blockIdx.x * 4 + wave) * 16;  // waves past the image still take part in the barriers
    const int p = strip + i16;
    const int py = p < a.npix ? p / a.w : -0x40000000;
    const int px = p - (p / a.w) * a.w;
    f32x4 acc[1][NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[0][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<f32x4 *>(a.in), 0, (a.in_g0 + a.c4) * a.npix * 16, 0x00020000);
    auto fetch = [&](f32x4 &xv, int S) {
        const int2 e = tab[S * 4 + g];
        const int dy = e.y >> 16, dx = (int)(short)(e.y & 0xffff);
        const bool ok = (unsigned)(py + dy) < (unsigned)a.h && (unsigned)(px + dx) < (unsigned)a.w;
        xv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? (unsigned)(e.x + p) * 16u : 0xffffffffu, 0, 0));
    };
    auto mac = [&](const f32x4 &xv, int sl) {
        f32x4 wv[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) wv[n] = wl[(sl * NT + n) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[n][j], xv[j], acc[0][n], 0, 0, 0);
    };
    f32x4 x0, x1, x2;
    fetch(x0, 0);
    fetch(x1, 1);
    const int nsp = a.nsteps + kPadSteps;
    for (int S = 0; S < a.nsteps; S += 3) {
        if (S) __syncthreads();
        for (int i = threadIdx.x; i < CS * NT * 64; i += 256) {  // chunk [S, S + 3) of every tile ([tile][superstep][lane] in memory)
            const int n = i / (CS * 64), r = i - n * (CS * 64);
            wl[((r >> 6) * NT + n) * 64 + (r & 63)] = a.wp[((size_t)n * nsp + S) * 64 + r];
        }
        __syncthreads();
        fetch(x2, S + 2);
        mac(x0, 0);
        fetch(x0, S + 3);
        mac(x1, 1);
        fetch(x1, S + 4);
        mac(x2, 2);
    }
    f32x4 bvec[NT], rvec[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        bvec[n] = *reinterpret_cast<const f32x4 *>(a.bias + (size_t)n * 16 + 4 * g);
        rvec[n] = f32x4{1.f, 1.f, 1.f, 1.f};
    }
    if (strip >= a.npix) return;
    conv_epilogue<1, NT>(a, acc, strip, i16, g, bvec, rvec);
}

// ------------------------------------------------------------------------------------------------
// Split-fp16 variant of the generic convolution (OJF_ARITH_F16X3).  Same C4-planar fp32 activations in
// and out; a superstep is one 32-wide K block = 8 (tap, 4-channel group) entries, lane group g owns
// entries 8S+2g and 8S+2g+1 (K slot j < 4: channel j of the first, j >= 4: channel j-4 of the second),
// converts its 8 fp32 values to fp16 halves in registers and issues 3 MFMAs per output tile.
// The packed weights ([S][n][hi|lo][lane] x 8 halfs) are staged through LDS in chunks of CS supersteps
// shared by the four waves of the block: with the 5x faster MFMA the per-wave L1 weight stream of the
// fp32 kernel would be the bound (measured: 35 -> 26 us on the grouped 19->19 3x3 launches).
// ------------------------------------------------------------------------------------------------
constexpr int conv16_chunk(int nt) { return nt <= 2 ? 6 : 3; }  // supersteps per LDS chunk (<= 24 KB)

// ABL: profiling-only ablation mask (tests/microbench): 1 = no activation loads, 2 = no LDS weight reads,
// 4 = no MFMA, 8 = no fp16 split.  Product launches always use ABL = 0.
// INS: the input planes are split planes (every convolution of the launch: the host checks)
template <int MT, int NT, bool SKIP = true, int ABL = 0, bool LEAN = false, bool INS = false>
// (the lean grouped 3x3 form keeps four waves per SIMD - 128 registers - now that its blocks are persistent: the pixel-block loop costs
// 12 registers, which without the bound dropped it to three)
__global__ __launch_bounds__(256, (MT == 2 && NT == 2 && LEAN) ? 4 : 1) void conv_f16x3_kernel(const ConvGroup grp)
{
    constexpr int CS = conv16_chunk(NT);
    const ConvArgs &a = grp.g[blockIdx.y];
    const bool persist = grp.band != 0;  // (uniform)
    int sb = grp.nblocks ? xcd_band_block(blockIdx.x, gridDim.x) : blockIdx.x;
    int sb_end = sb + 1, sb_step = 1;
    if (persist) {  // block j of XCD x walks positions j, j + P, j + 2 P .. of the XCD's band [x band, (x + 1) band)
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        sb = x * grp.band + j;
        sb_end = (x + 1) * grp.band;
        sb_step = (int)(gridDim.x >> 3);
    }
    if (grp.nblocks && sb >= grp.nblocks) return;  // padding block of a banded launch
    extern __shared__ int2 tab[];  // (nsteps + kPad16) * 8 entries, sized by the launch: LDS per block bounds the waves in flight
    __shared__ f32x4 wl[CS * NT * 128];
    build_tap_table16(tab, a, (a.nsteps + kPad16) * 8);
    if (persist) {  // the layer's weights are one chunk (the host checks): copied once for all of the block's pixel blocks
#pragma unroll
        for (int i = 0; i < CS * NT * 128 / 256; ++i) wl[i * 256 + threadIdx.x] = a.wp[i * 256 + threadIdx.x];
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    __syncthreads();  // tap table (and the persistent form's weights)
    for (; sb < sb_end && (!grp.nblocks || sb < grp.nblocks); sb += sb_step) {
    int strip = (sb * 4 + wave) * (MT * 16);  // waves past the image still take part in the barriers
    if (a.row_perm) {  // (the host sets it only when w is a multiple of MT * 16: a wave's pixel tiles lie in one row)
        const int pr = fast_div(strip, a.w, a.w_magic);
        if (pr < a.h) strip = perm_row(pr, a.row_perm, a.perm_q, a.perm_rem) * a.w + (strip - pr * a.w);
    }

    // vm: bit t set <=> tap t of this lane's pixel lies inside the image (bit 0 only for 1x1); p16: byte offset
    int p16[MT];
    unsigned vm[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int p = strip + m * 16 + i16;
        p16[m] = p * 16;
        const int py = fast_div(p, a.w, a.w_magic), px = p - py * a.w;
        unsigned rm = 0, cm = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            rm |= ((unsigned)(py + (k - 1) * a.dil) < (unsigned)a.h ? 1u : 0u) << k;
            cm |= ((unsigned)(px + (k - 1) * a.dil) < (unsigned)a.w ? 1u : 0u) << k;
        }
        const unsigned all9 = ((rm & 1u) ? cm : 0u) | ((rm & 2u) ? cm << 3 : 0u) | ((rm & 4u) ? cm << 6 : 0u);
        vm[m] = p < a.npix ? (a.taps == 9 ? all9 : 1u) : 0u;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            // MT = 1: the zeros are made opaque, so that every MFMA accumulates in place.  Left to itself clang folds them into
            // the first MFMA of the peeled first superstep (SrcC = 0) and, at NT >= 6, sends tile 0 through a scratch tuple
            // (a[0:3] = W_lo X_hi; a[0:3] += W_hi X_lo; a[8:11] = W_hi X_hi + a[0:3], next tile's first MFMA into a[0:3]
            // right behind): on MI355X that tile came out without its low-half products (2e-4 instead of 2e-6) or as NaN
            // (tests/test_net_gpu.py::test_conv2d_layer at 114 -> 95 and 19 -> 114 caught it when the wide launches moved to
            // MT = 1); the same back-to-back shapes occur in kernels that are right, so this is pinned by test, not by rule.
            if constexpr (MT == 1) asm volatile("" : "+v"(acc[m][n]));
        }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<f32x4 *>(a.in), 0, (a.in_g0 + a.c4) * a.npix * 16, 0x00020000);
    // bias and inverse row scale of the epilogue: for the narrow layers they are fetched here, so that their latency
    // hides behind the main loop (the wide ones cannot afford the registers: 268 VGPRs at NT = 8)
    constexpr bool kHoist = NT <= 4;
    f32x4 bvec[NT], rvec[NT];
    if constexpr (kHoist) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            bvec[n] = *reinterpret_cast<const f32x4 *>(a.bias + (size_t)n * 16 + 4 * g);
            rvec[n] = *reinterpret_cast<const f32x4 *>(a.rinv + (size_t)n * 16 + 4 * g);
        }
    }

    // Operand fetch of superstep S: two (tap, channel group) entries per lane group.  The 9 taps' in-image tests
    // are one bit each in vm[] (computed once per wave), so an entry costs and + compare + add + select; buffer
    // loads return zeros for the out-of-range offset of an invalid tap.
    const int4 *tab4 = reinterpret_cast<const int4 *>(tab) + g;  // lane group g's two entries of a superstep
    auto fetch = [&](f32x4(&xa)[MT], f32x4(&xb)[MT], const int4 e, bool &live) {
        unsigned any = 0;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const unsigned o0 = (unsigned)(e.x + p16[m]) | ((vm[m] & (unsigned)e.y) ? 0u : 0xffffffffu);
            const unsigned o1 = (unsigned)(e.z + p16[m]) | ((vm[m] & (unsigned)e.w) ? 0u : 0xffffffffu);
            if constexpr (ABL & 1) {
                xa[m] = f32x4{1.f, 2.f, 3.f, 4.f};
                xb[m] = f32x4{1.f, 2.f, 3.f, 4.f};
                asm volatile("" ::"v"(o0), "v"(o1));
            } else {
                xa[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o0, 0, 0));
                xb[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o1, 0, 0));
            }
            any |= vm[m] & (unsigned)(e.y | e.w);
        }
        live = SKIP ? __any(any != 0) : true;  // dead superstep: every source pixel of the wave is outside the image
    };
    auto mac = [&](const f32x4(&xa)[MT], const f32x4(&xb)[MT], int sl) {
        f32x4 wh[NT], wlo[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            if constexpr (ABL & 2) {
                wh[n] = wlo[n] = f32x4{1.f, 1.f, 1.f, 1.f};
                asm volatile("" ::"s"(sl));
            } else {
                wh[n] = wl[(sl * NT + n) * 128 + lane];
                wlo[n] = wl[(sl * NT + n) * 128 + 64 + lane];
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            f16x8 xh, xl;
            if constexpr (ABL & 8) {
                xh = __builtin_bit_cast(f16x8, xa[m]);
                xl = __builtin_bit_cast(f16x8, xb[m]);
            } else if constexpr (INS) {
                unpack_split(xa[m], xb[m], xh, xl);
            } else {
                split_f16(xa[m], xb[m], xh, xl);
            }
            if constexpr (ABL & 4) {
                asm volatile("" ::"v"(xh), "v"(xl));
#pragma unroll
                for (int n = 0; n < NT; ++n) asm volatile("" ::"v"(wh[n]), "v"(wlo[n]));
            } else {
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = mfma_f16x3(wh[n], wlo[n], xh, xl, acc[m][n]);
            }
        }
    };

    f32x4 xa0[MT], xb0[MT], xa1[MT], xb1[MT], xa2[MT], xb2[MT];
    bool v0, v1, v2;
    fetch(xa0, xb0, tab4[0], v0);
    fetch(xa1, xb1, tab4[4], v1);
    int sl = persist ? 0 : CS;
    for (int S = 0; S < a.nsteps; S += 3) {
        // the three table reads of this iteration are issued together (one LDS latency instead of three)
        const int4 t2 = tab4[(S + 2) * 4], t3 = tab4[(S + 3) * 4], t4 = tab4[(S + 4) * 4];
        if (sl == CS) {  // next weight chunk (CS is a multiple of the 3 supersteps of one iteration)
            // plain copy: prefetching the chunk through registers one chunk ahead measured slower on the wide and
            // the grouped launches (17.9 -> 20.7 us, 23.1 -> 25.1 us: VGPRs) and equal elsewhere
            if (S) __syncthreads();
            const f32x4 *src = a.wp + (size_t)S * NT * 128;
#pragma unroll
            for (int i = 0; i < CS * NT * 128 / 256; ++i) wl[i * 256 + threadIdx.x] = src[i * 256 + threadIdx.x];
            __syncthreads();
            sl = 0;
        }
        fetch(xa2, xb2, t2, v2);
        if (!SKIP || v0) mac(xa0, xb0, sl);
        fetch(xa0, xb0, t3, v0);
        if (!SKIP || v1) mac(xa1, xb1, sl + 1);
        fetch(xa1, xb1, t4, v1);
        if (!SKIP || v2) mac(xa2, xb2, sl + 2);
        sl += 3;
    }
    if constexpr (!kHoist) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            bvec[n] = *reinterpret_cast<const f32x4 *>(a.bias + (size_t)n * 16 + 4 * g);
            rvec[n] = *reinterpret_cast<const f32x4 *>(a.rinv + (size_t)n * 16 + 4 * g);
        }
    }
    if constexpr (LEAN) {
        int tile0[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) tile0[m] = strip + m * 16;
        conv_epilogue_lean<MT, NT>(a, acc, tile0, i16, g, bvec, rvec);
    } else {
        conv_epilogue<MT, NT, true>(a, acc, strip, i16, g, bvec, rvec);
    }
    }  // (pixel blocks of a persistent block)
}

// ------------------------------------------------------------------------------------------------
// Row-pair form of the banded, lean, split-plane grouped 3x3 launches (the four branches' dilated 19 -> 19 convolutions).
// conv_f16x3_kernel gives a wave 32 consecutive pixels of one row: its two tiles fetch three tap rows each, "every operand
// once per tap" (24 one-KB loads per wave).  Here a wave's two tiles are the same 16 columns of two rows that are neighbours in
// the launch's row order - (y mod r, y div r) under row_perm, y otherwise - i.e. `dil` apart inside a dilation class: each is a
// tap row of the other, so the pair reads FOUR source rows instead of six (16 loads), and the registers of tile 1's row are
// tile 0's operands one tap row later.  Pairs that are not `dil` apart (a pair straddling two classes, dil >= h) run the same
// code on six rows.
//   band position sb -> pair k = sb / (w / 64), column group c = sb % (w / 64); wave v owns columns 64 c + 16 v .. + 15;
//   tile m is row perm_row(2 k + m) (plain 2 k + m without row_perm).  With w % 64 == 0 and h even (the host checks) there
//   are (h / 2)(w / 64) positions - the very nblocks of the old form: grid, bands and the persistent walk are the same.
// K is walked by tap row ky = 0, 1, 2, two supersteps of 16 slots each, slot = kx * c4 + cg (3 c4 <= 16; the slots behind
// are dead: zero weights, their loads masked out of range): lane group g owns slots 2g, 2g + 1 of the first and 8 + 2g,
// 9 + 2g of the second superstep - four float4 (16 registers) per source row, whose plane offsets and tap columns never
// change: no tap table.
// The weights are a stream of their own (PackedConv::wp_rows, 6 supersteps = 24 KB, copied to LDS once per block).
// A pixel's sum does not depend on the path: both accumulate ky = 0, 1, 2 from the same fragments and skip exactly the
// tap rows outside the image (no loads, no MFMAs).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 3) void conv_f16x3_rows_kernel(const ConvGroup grp)
{
    constexpr int NT = 2, CS = 6;
    const ConvArgs &a = grp.g[blockIdx.y];
    int sb = xcd_band_block(blockIdx.x, gridDim.x);
    int sb_end = sb + 1, sb_step = 1;
    if (grp.band) {  // persistent: as in conv_f16x3_kernel
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
        sb = x * grp.band + j;
        sb_end = (x + 1) * grp.band;
        sb_step = (int)(gridDim.x >> 3);
    }
    if (sb >= grp.nblocks) return;  // padding block
    __shared__ f32x4 wl[CS * NT * 128];
#pragma unroll
    for (int i = 0; i < CS * NT * 128 / 256; ++i) wl[i * 256 + threadIdx.x] = a.wp_rows[i * 256 + threadIdx.x];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    // this lane's four slots: byte offset of (plane, tap column) relative to the pixel, and the tap column's bit (0: dead slot)
    int soff[4];
    unsigned sbit[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int slot = (j >> 1) * 8 + 2 * g + (j & 1);
        const int kx = fast_div(slot, a.c4, a.c4_magic), cg = slot - kx * a.c4;
        const bool on = kx < 3;
        soff[j] = on ? ((a.in_g0 + cg) * a.npix + (kx - 1) * a.dil) * 16 : 0;
        sbit[j] = on ? 1u << kx : 0u;
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<f32x4 *>(a.in), 0, (a.in_g0 + a.c4) * a.npix * 16, 0x00020000);
    f32x4 bvec[NT], rvec[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        bvec[n] = *reinterpret_cast<const f32x4 *>(a.bias + (size_t)n * 16 + 4 * g);
        rvec[n] = *reinterpret_cast<const f32x4 *>(a.rinv + (size_t)n * 16 + 4 * g);
    }
    const int cgroups = a.w >> 6;
    __syncthreads();  // the weights

    for (; sb < sb_end && sb < grp.nblocks; sb += sb_step) {
        const int k = sb / cgroups, px = (sb - k * cgroups) * 64 + wave * 16 + i16;
        int row0 = 2 * k, row1 = 2 * k + 1;
        if (a.row_perm) {
            row0 = perm_row(row0, a.row_perm, a.perm_q, a.perm_rem);
            row1 = perm_row(row1, a.row_perm, a.perm_q, a.perm_rem);
        }
        unsigned cm = 0;  // bit kx: tap column kx of this lane's pixel lies inside the image
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) cm |= ((unsigned)(px + (kx - 1) * a.dil) < (unsigned)a.w ? 1u : 0u) << kx;
        unsigned sinv[4];  // all ones for a slot that reads nothing: the buffer load then returns zeros
#pragma unroll
        for (int j = 0; j < 4; ++j) sinv[j] = (cm & sbit[j]) ? 0u : 0xffffffffu;

        // one source row: four loads per lane; a row outside the image costs nothing (and is never consumed)
        auto fetch = [&](f32x4(&x)[4], int r) {
            if ((unsigned)r < (unsigned)a.h) {
                const int p16 = (r * a.w + px) * 16;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    x[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(soff[j] + p16) | sinv[j], 0, 0));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        f32x4 acc[2][NT];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        // tap row ky: tile 0 consumes source row x0 (if it lies inside the image: on0), tile 1 x1 - the same weight fragments
        auto mac = [&](int ky, const f32x4(&x0)[4], bool on0, const f32x4(&x1)[4], bool on1) {
            if (!on0 && !on1) return;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f32x4 wh[NT], wlo[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    wh[n] = wl[((ky * 2 + s) * NT + n) * 128 + lane];
                    wlo[n] = wl[((ky * 2 + s) * NT + n) * 128 + 64 + lane];
                }
                f16x8 xh, xl;
                if (on0) {
                    unpack_split(x0[2 * s], x0[2 * s + 1], xh, xl);
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc[0][n] = mfma_f16x3(wh[n], wlo[n], xh, xl, acc[0][n]);
                }
                if (on1) {
                    unpack_split(x1[2 * s], x1[2 * s + 1], xh, xl);
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc[1][n] = mfma_f16x3(wh[n], wlo[n], xh, xl, acc[1][n]);
                }
            }
        };
        auto inside = [&](int r) { return (unsigned)r < (unsigned)a.h; };
        const int d = a.dil;
        f32x4 xa[4], xb[4], xc[4], xd[4];
        if (row1 == row0 + d) {  // (wave-uniform) four source rows: row0 - d, row0, row1, row1 + d
            fetch(xa, row0 - d);
            fetch(xb, row0);
            fetch(xc, row1);
            fetch(xd, row1 + d);
            mac(0, xa, inside(row0 - d), xb, true);
            mac(1, xb, true, xc, true);
            mac(2, xc, true, xd, inside(row1 + d));
        } else {  // independent tiles: six source rows
            fetch(xa, row0 - d);
            fetch(xb, row1 - d);
            fetch(xc, row0);
            fetch(xd, row1);
            mac(0, xa, inside(row0 - d), xb, inside(row1 - d));
            fetch(xa, row0 + d);
            fetch(xb, row1 + d);
            mac(1, xc, true, xd, true);
            mac(2, xa, inside(row0 + d), xb, inside(row1 + d));
        }
        const int tile0[2] = {row0 * a.w + px - i16, row1 * a.w + px - i16};
        conv_epilogue_lean<2, NT>(a, acc, tile0, i16, g, bvec, rvec);
    }
}

// ------------------------------------------------------------------------------------------------
// Fused 1x1 chain (the prediction head, model.py:24-52,252-256): 11 pointwise layers in ONE launch.
// With weights as the MFMA A operand, the accumulator of lane (pixel i, g) for output tile n holds
// channels 16n+4g..+3 of its pixel - exactly the B-operand fragment (channel group 4S+g, S = n) the
// next layer needs.  Activations therefore never leave registers between layers: each layer is
//   nxt[n2] = sum_S sum_j mfma(W_l[n2][S][j], act(cur[S])[j]),
// only the weights stream, and they are staged per layer (in <= 24 KB parts) through LDS so that the
// four waves of a block share one fetch.  Tile counts are compile-time (two supported topologies:
// 19- and 20-channel growth), so every register array is statically indexed.
// ------------------------------------------------------------------------------------------------
constexpr int kChainLdsFloat4 = 48 * 1024 / 16;
constexpr int kChainDmaHalf = 1536;  // float4 per half of the split-fp16 weight double buffer

struct ChainArgs {
    const f32x4 *in;  // input planes, c4_in groups starting at in_g0
    const f32x4 *w;   // per layer: [n2 < NTOUT][K block][lane] fragments (see chain_unit), layers back to back
    const float *bias;  // per layer NTOUT*16 floats, back to back
    float *out_rows;  // [npix, rows_stride], channels < rows_n
    int in_g0, c4_in, npix, rows_stride, rows_n;
    float scale;
    int *ovf;  // split-fp16 range guard flag (see ConvArgs)
    // kChainEntry (branch-entry GEMM of a VortexPooling run on register-resident input): result planes
    f32x4 *out_planes;
    int out_g0, og_store, act_n;  // ReLU on channels < act_n (branch 0), the pooled branches stay linear
    struct ColSums *colsum;       // channel sums of the entry layer's INPUT (global-average branch), see block_colsum
    int in_split = 0;             // entry1x1_kernel: the input planes are split planes (the dense-growth buffer of dense_chain_kernel)
    int split_groups = 0;         // kChainEntry: channel groups < split_groups (branch 0, read by its 3x3 convolution only) are stored as split planes
#ifdef OJF_ENTRY_STAMPS
    int stamp = 0;                // the stand-alone entry GEMM's launches set it: the fused tail's entry layer leaves the stamps alone
#endif
};

#ifdef OJF_ENTRY_STAMPS  // profiling build only (tools/entry_stamps.py): phase stamps of the stand-alone entry GEMM's blocks, thread 0
// [block][strip of the block's walk < 4][slot]: clock64 at 0 strip start (block start for the first), 1 inputs landed, 2 channel sums
// done, 3 weight part 0 landed (persistent form: the whole layer, first strip only), 4 weight part 1 landed (one-strip form only),
// 5 MFMAs issued, 6 stores issued; 100-MHz wall clock at 7 strip start, 8 strip end; 9 = strip index + 1.  In the persistent form a
// strip's planes land while the strip before it computes: its slot 1 then precedes its slot 0.  The stamps of the LAST stamped launch remain.
constexpr int kEntryStampBlocks = 8192, kEntryStampStrips = 4, kEntryStampSlots = 10;
__device__ unsigned long long g_entry_stamps[kEntryStampBlocks][kEntryStampStrips][kEntryStampSlots];
#define ENTRY_STAMP(on, k, i, v)                                                                                              \
    do {                                                                                                                       \
        if ((on) && threadIdx.x == 0 && blockIdx.x < (unsigned)kEntryStampBlocks && (k) < kEntryStampStrips)                   \
            g_entry_stamps[blockIdx.x][k][i] = (i) == 9 ? (unsigned long long)(v) : ((i) >= 7 ? wall_clock64() : clock64());   \
    } while (0)
#define ENTRY_STAMP_ON(a) ((a).stamp)
#define ENTRY_STAMP_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")  // "inputs landed" has to wait for them (the one-strip form)
#else
#define ENTRY_STAMP(on, k, i, v) do { } while (0)
#define ENTRY_STAMP_ON(a) 0
#define ENTRY_STAMP_LANDED() do { } while (0)
#endif

// Weight fragments of one (output tile, K block) pair.  fp32: K block = one 16-channel input tile, 64 float4
// (lane (oc i16, g) holds W[oc][16S+4g .. +3]).  split-fp16: K block = two input tiles (32 channels), 128 float4 =
// hi | lo fragments of 8 halfs; K slot j < 4 is channel 4g+j of tile 2S', j >= 4 channel 4g+j-4 of tile 2S'+1 - i.e.
// exactly the two accumulator quads lane (pixel, g) holds, so activations still never leave registers.
constexpr int chain_kblocks(int arith, int ntin) { return arith == OJF_ARITH_F16X3 ? (ntin + 1) / 2 : ntin; }
constexpr int chain_unit(int arith) { return arith == OJF_ARITH_F16X3 ? 128 : 64; }
constexpr int chain_layer_size(int arith, int ntin, int ntout) { return ntout * chain_kblocks(arith, ntin) * chain_unit(arith); }
// How the weight parts reach LDS:
//   fp32:       global -> registers (`pre`, issued one part ahead) -> ds_write, one 48 KB buffer, two barriers per part
//   split-fp16: LDS-DMA (global_load_lds_dwordx4, 1 KB per wave instruction) straight into the other half of a
//               2 x 24 KB double buffer while the current part computes: no staging registers (48 VGPRs less, which
//               is what lets more waves hide the LDS latency of the 5x faster MFMA phase), no ds_write pass, one
//               barrier per part.
constexpr bool chain_dma(int arith) { return arith == OJF_ARITH_F16X3; }
constexpr int chain_cap(int arith) { return chain_dma(arith) ? kChainDmaHalf : kChainLdsFloat4; }  // float4 per part
// output tiles per LDS part: as many whole tiles as fit; parts = the number of such groups
constexpr int chain_tiles_fit(int arith, int ntin)
{
    return chain_cap(arith) / (chain_kblocks(arith, ntin) * chain_unit(arith));
}
constexpr int chain_parts(int arith, int ntin, int ntout)
{
    return (ntout + chain_tiles_fit(arith, ntin) - 1) / chain_tiles_fit(arith, ntin);
}
constexpr int chain_per(int arith, int ntin, int ntout)
{   // balanced over the parts (a part never exceeds chain_tiles_fit)
    return (ntout + chain_parts(arith, ntin, ntout) - 1) / chain_parts(arith, ntin, ntout);
}
constexpr int chain_first_size(int arith, int ntin, int ntout)
{   // float4 count of a layer's first part
    return (chain_per(arith, ntin, ntout) < ntout ? chain_per(arith, ntin, ntout) : ntout) * chain_kblocks(arith, ntin) *
           chain_unit(arith);
}
// per-layer floats in the bias stream: bias[NTOUT*16], and for split-fp16 the inverse row scales behind it
constexpr int chain_bias_stride(int arith, int ntout) { return (arith == OJF_ARITH_F16X3 ? 2 : 1) * ntout * 16; }
constexpr int kChainAhead = 2;  // weight fragments requested ahead of their MFMAs (split-fp16 chain layers)
constexpr int kChainWaves = 4, kChainThreads = 64 * kChainWaves;  // waves of a chain / tail / entry block
constexpr int kChainBlocks = 3;  // blocks of them a CU is to hold (launch bound)
constexpr int kChainPre = kChainLdsFloat4 / kChainThreads;  // float4 registers per thread holding the prefetched next part

// LDS-DMA of `size` float4 (a multiple of 64) from src to the LDS address dst: wave w moves the 1 KB chunks
// w, w+4, ...; completion = this wave's vmcnt reaching 0, visibility to the block = the barrier after that
__device__ __forceinline__ void dma_part(const f32x4 *src, f32x4 *dst, int size, int wave, int lane)
{
#pragma unroll
    for (int c0 = 0; c0 < kChainDmaHalf / 64; c0 += kChainWaves) {
        const int c = c0 + wave;
        if (c * 64 < size)
            __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)(src + c * 64 + lane),
                                             (void __attribute__((address_space(3))) *)(dst + c * 64), 16, 0, 0);
    }
}

enum { kChainLeaky = 0, kChainRelu = 1, kChainAccumulate = 2, kChainLastRows = 3, kChainEntry = 4 };

// Epilogue vectors (bias | inverse row scale, chain_bias_stride floats per layer) travel one layer ahead of their use:
// threads < n fetch one float4 each of the NEXT epilogue-bearing layer while the current layer computes (vec_issue),
// write it into one half of a 2 x 1 KB LDS buffer at that layer's entry (vec_commit; the layer's first barrier publishes
// it), and the epilogue reads its four float4 per output tile from LDS.  Fetching them from global memory inside the
// epilogue put an L2 round trip at the end of every layer of every wave (measured with the loads ablated: tail + head
// 84 -> 73 us, tail + entry 64 -> 59 us).
constexpr int kVecF4 = 64;  // float4 per half: 8 output tiles x (4 bias + 4 scale)
struct VecStage {
    f32x4 *lds;  // [2][kVecF4]
    f32x4 reg;   // this thread's float4 of the staged layer (threads < its float4 count)
    int half;    // half the next commit writes
};
struct VecNext {  // where the next layer's vectors come from: na float4 at a, then nb float4 at b (either may be empty)
    const float *a = nullptr;
    int na = 0;
    const float *b = nullptr;
    int nb = 0;
};
__device__ __forceinline__ void vec_issue(VecStage &vs, const VecNext &nx)
{
    const int t = threadIdx.x;
    if (t < nx.na) vs.reg = reinterpret_cast<const f32x4 *>(nx.a)[t];
    else if (t < nx.na + nx.nb) vs.reg = reinterpret_cast<const f32x4 *>(nx.b)[t - nx.na];
}
// returns the base of the half now holding the vectors (valid for every thread after the next barrier)
__device__ __forceinline__ const f32x4 *vec_commit(VecStage &vs, int n)
{
    f32x4 *dst = vs.lds + vs.half * kVecF4;
    if ((int)threadIdx.x < n) dst[threadIdx.x] = vs.reg;
    vs.half ^= 1;
    return dst;
}

// One pointwise layer on register-resident activations: out[n2] (+)= sum_K W[n2][K] * in[K], then (unless
// accumulating) bias + activation in place.  `in` and `out` are distinct, statically indexed register arrays
// (callers ping-pong two of them), so no staging copy exists.
// `pre` carries the weights of this layer's first part on entry (already fetched from HBM/L2 while the
// previous part computed) and the next layer's first part on exit: global latency never sits between two
// compute phases, only the two barriers around the LDS refill do.
struct ChainNoHook { __device__ __forceinline__ void operator()() const {} };
template <int ARITH, int MT, int NTIN, int NTOUT, int MODE, int NEXT_FIRST, int NA, int NB, class HOOK = ChainNoHook>
__device__ __forceinline__ void chain_layer(const f32x4 (&in)[MT][NA], f32x4 (&out)[MT][NB], f32x4 *wlds, const f32x4 *wg,
                                            const ChainArgs &a, const int (&p)[MT], int lane,
                                            f32x4 (&pre)[kChainPre], int &buf, VecStage &vs, const VecNext nx = VecNext(),
                                            const f32x4 *next_src = nullptr, int commit_extra = 0, HOOK hook = HOOK())
{
    static_assert(NTIN <= NA && NTOUT <= NB, "register arrays too small for this layer");
    // this layer's epilogue vectors (issued one layer ago) go to LDS now; an accumulating layer may carry the vectors of
    // the code that follows it (commit_extra).  The first barrier below publishes them.
    const f32x4 *vec = vec_commit(vs, MODE != kChainAccumulate ? chain_bias_stride(ARITH, NTOUT) / 4 : commit_extra);
    constexpr int parts = chain_parts(ARITH, NTIN, NTOUT);
    constexpr int per = chain_per(ARITH, NTIN, NTOUT);
    constexpr int KB = chain_kblocks(ARITH, NTIN);
    constexpr int unit = chain_unit(ARITH);
    static_assert(per * KB * unit <= chain_cap(ARITH), "LDS part too large");
    // split-fp16: the fp16 halves of the layer input, once per layer
    f16x8 xh[MT][ARITH == OJF_ARITH_F16X3 ? KB : 1], xl[MT][ARITH == OJF_ARITH_F16X3 ? KB : 1];
    if constexpr (ARITH == OJF_ARITH_F16X3) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int S = 0; S < KB; ++S) {
                const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
                split_f16(in[m][2 * S], 2 * S + 1 < NTIN ? in[m][2 * S + 1 < NTIN ? 2 * S + 1 : 0] : zero, xh[m][S], xl[m][S]);
            }
    }
#pragma unroll
    for (int part = 0; part < parts; ++part) {
        const int nb = part * per;
        const int ne = nb + per < NTOUT ? nb + per : NTOUT;
        const int size = (ne - nb) * KB * unit;
        // the following part (next part of this layer, or the next layer's first)
        const int nnb = ne;
        const int nne = nnb + per < NTOUT ? nnb + per : NTOUT;
        const int nsize = part + 1 < parts ? (nne - nnb) * KB * unit : NEXT_FIRST;
        const f32x4 *nsrc = part + 1 < parts ? wg + (size_t)nnb * KB * unit
                                             : (next_src ? next_src : wg + (size_t)chain_layer_size(ARITH, NTIN, NTOUT));
        const f32x4 *wpart = wlds;
        if constexpr (chain_dma(ARITH)) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's chunks of the current part have landed
            __syncthreads();  // ... everybody's have, and the readers of the other buffer are done with it
            if constexpr (MODE == kChainEntry) ENTRY_STAMP(ENTRY_STAMP_ON(a) && part < 2, 0, 3 + (part < 2 ? part : 0), 0);
            wpart = wlds + buf * chain_cap(ARITH);
            buf ^= 1;
            dma_part(nsrc, wlds + buf * chain_cap(ARITH), nsize, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane);
            if (part == 0) vec_issue(vs, nx);
            if (part == 0) hook();  // (requests of the caller's that are to travel behind the layer's first barrier)
        } else {
            __syncthreads();  // readers of the previous part are done
#pragma unroll
            for (int k = 0; k < kChainPre; ++k)
                if ((int)threadIdx.x + kChainThreads * k < size) wlds[threadIdx.x + kChainThreads * k] = pre[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kChainPre; ++k)
                if ((int)threadIdx.x + kChainThreads * k < nsize) pre[k] = nsrc[threadIdx.x + kChainThreads * k];
            if (part == 0) vec_issue(vs, nx);
            if (part == 0) hook();  // (requests of the caller's that are to travel behind the layer's first barrier)
        }
        if constexpr (MODE != kChainAccumulate) {
#pragma unroll
            for (int n2 = 0; n2 < NTOUT; ++n2)
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    if (n2 >= nb && n2 < ne) out[m][n2] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // K block outer, output tiles inner: (ne - nb) * MT independent accumulators per MFMA round
        if constexpr (ARITH == OJF_ARITH_F16X3) {
            // Software pipeline over the part's (K block, output tile) steps: the weight fragments of step t + kChainAhead
            // are requested from LDS before the MFMAs of step t are issued.  Left alone, the compiler sinks every
            // ds_read next to its use (read -> s_waitcnt lgkmcnt(0) -> 3 MFMAs): ~100 cycles of LDS latency per 48
            // cycles of matrix work, the "parked" half of this kernel's wave-cycles.
            const int cnt = ne - nb, steps = KB * cnt;
            f32x4 rh[kChainAhead], rl[kChainAhead];
            auto frag = [&](int t) { return ((t % cnt) * KB + t / cnt) * 128; };  // step t = (S = t / cnt, tile nb + t % cnt)
#pragma unroll
            for (int t = 0; t < kChainAhead; ++t)
                if (t < steps) {
                    rh[t] = wpart[frag(t) + lane];
                    rl[t] = wpart[frag(t) + 64 + lane];
                }
#pragma unroll
            for (int t = 0; t < KB * NTOUT; ++t) {
                if (t >= steps) break;
                const f32x4 wh = rh[t % kChainAhead], wl = rl[t % kChainAhead];
                if (t + kChainAhead < steps) {
                    rh[t % kChainAhead] = wpart[frag(t + kChainAhead) + lane];
                    rl[t % kChainAhead] = wpart[frag(t + kChainAhead) + 64 + lane];
                }
                __builtin_amdgcn_sched_barrier(0);
                const int S = t / cnt, n2 = nb + t % cnt;
#pragma unroll
                for (int m = 0; m < MT; ++m) out[m][n2] = mfma_f16x3(wh, wl, xh[m][S], xl[m][S], out[m][n2]);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
        for (int S = 0; S < KB; ++S)
#pragma unroll
            for (int n2 = 0; n2 < NTOUT; ++n2) {
                if (n2 < nb || n2 >= ne) continue;
                {
                    const f32x4 wv = wpart[((n2 - nb) * KB + S) * 64 + lane];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            out[m][n2] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[j], in[m][S][j], out[m][n2], 0, 0, 0);
                }
            }
        }
    }
    if constexpr (MODE == kChainEntry) ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 5, 0);
    if constexpr (MODE != kChainAccumulate) {
        const int g = lane >> 4;
        float gmax = 0.0f;
#pragma unroll
        for (int n2 = 0; n2 < NTOUT; ++n2) {
            const f32x4 b = vec[n2 * 4 + g];
            f32x4 ri{1.f, 1.f, 1.f, 1.f};
            if constexpr (ARITH == OJF_ARITH_F16X3) ri = vec[(NTOUT + n2) * 4 + g];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const f32x4 lin4 = ARITH == OJF_ARITH_F16X3 ? fma4(out[m][n2], ri, b) : out[m][n2] + b;
                f32x4 v = lin4;
                if constexpr (MODE == kChainLastRows) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int oc = n2 * 16 + 4 * g + j;
                        if (oc < a.rows_n && p[m] < a.npix)
                            a.out_rows[(size_t)p[m] * a.rows_stride + oc] = tanhf(v[j]) * a.scale;
                    }
                } else if constexpr (MODE == kChainEntry) {
                    const int og = n2 * 4 + g;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (og * 4 + j < a.act_n && !(v[j] > 0.0f)) ? (v[j] != v[j] ? v[j] : 0.0f) : v[j];
                    if (p[m] < a.npix && og < a.og_store) {
                        a.out_planes[(size_t)(a.out_g0 + og) * a.npix + p[m]] = og < a.split_groups ? split_pack4(v) : v;
                        if constexpr (ARITH == OJF_ARITH_F16X3) gmax = guard_max(gmax, lin4);
                    }
                } else {
                    constexpr float slope = MODE == kChainRelu ? 0.0f : 0.01f;
                    v = leaky_max4(v, slope);
                    if constexpr (ARITH == OJF_ARITH_F16X3) gmax = guard_max(gmax, lin4);  // pre-activation magnitude
                    out[m][n2] = v;
                }
            }
        }
        if constexpr (ARITH == OJF_ARITH_F16X3)
            if (gmax > 65504.0f && a.ovf) guard_raise(a.ovf, 1);
        if constexpr (MODE == kChainEntry) {
            ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 6, 0);
            ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 8, 0);
        }
    }
}

#ifdef OJF_TAIL_STAMPS  // profiling build only (tools/tail_stamps.py): phase stamps of the fused tails' blocks, thread 0
// [launch kind: 0 = tail + entry layer (or alone), 1 = tail + head][block][slot]: clock64 at 0 block start; for branch b at 1 + 3b inputs
// landed (the profiling build's own vmcnt(0) in front of the closing 1x1: the wave's planes AND its chunks of the weight part), 2 + 3b closing
// 1x1 done, 3 + 3b accumulation done; 13 final epilogue done, 14 channel sums done (tail + entry), 15 fused entry layer / head done; 100-MHz
// wall clock at 16 block start, 17 block end; 18 = block index + 1; 100-MHz wall clock at 20 + l: layer l < 11 of the prediction head done (chain_run).  The stamps
// of the LAST launch of each kind remain.
constexpr int kTailStampBlocks = 8192, kTailStampSlots = 32;
__device__ unsigned long long g_tail_stamps[2][kTailStampBlocks][kTailStampSlots];
#define TAIL_STAMP(kind, i, v)                                                                                                 \
    do {                                                                                                                       \
        if (threadIdx.x == 0 && blockIdx.x < (unsigned)kTailStampBlocks)                                                       \
            g_tail_stamps[kind][blockIdx.x][i] = (i) == 18 ? (unsigned long long)(v) : ((i) >= 16 ? wall_clock64() : clock64()); \
    } while (0)
#define TAIL_STAMP_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")  // "inputs landed" has to wait for them
#else
#define TAIL_STAMP(kind, i, v) do { } while (0)
#define TAIL_STAMP_LANDED() do { } while (0)
#endif

// layer l reads `x` and writes `y`; the recursion swaps the two arrays for layer l+1
template <int ARITH, int MT, int NTIN, int NTOUT>
__device__ __forceinline__ void chain_run(f32x4 (&x)[MT][8], f32x4 (&y)[MT][8], f32x4 *wlds, const f32x4 *wg,
                                          const float *bias, const ChainArgs &a, const int (&p)[MT], int lane,
                                          f32x4 (&pre)[kChainPre], int &buf, VecStage &vs)
{
    chain_layer<ARITH, MT, NTIN, NTOUT, kChainLastRows, 0>(x, y, wlds, wg, a, p, lane, pre, buf, vs);
    TAIL_STAMP(1, 30, 0);  // (chain_run serves the tails' prediction head only: 11 layers, this one the last)
}

template <int ARITH, int MT, int NTIN, int NTOUT, int NTNEXT, int... REST>
__device__ __forceinline__ void chain_run(f32x4 (&x)[MT][8], f32x4 (&y)[MT][8], f32x4 *wlds, const f32x4 *wg,
                                          const float *bias, const ChainArgs &a, const int (&p)[MT], int lane,
                                          f32x4 (&pre)[kChainPre], int &buf, VecStage &vs)
{
    // `bias` = this layer's vectors (already issued by the caller / the previous layer); the next layer's follow them
    VecNext nx;
    nx.a = bias + chain_bias_stride(ARITH, NTOUT);
    nx.na = chain_bias_stride(ARITH, NTNEXT) / 4;
    chain_layer<ARITH, MT, NTIN, NTOUT, kChainLeaky, chain_first_size(ARITH, NTOUT, NTNEXT)>(x, y, wlds, wg, a, p, lane, pre,
                                                                                             buf, vs, nx);
    TAIL_STAMP(1, 29 - (int)sizeof...(REST), 0);  // layer 9 - sizeof...(REST) of the head's 11
    chain_run<ARITH, MT, NTOUT, NTNEXT, REST...>(y, x, wlds, wg + (size_t)chain_layer_size(ARITH, NTIN, NTOUT),
                                                 bias + chain_bias_stride(ARITH, NTOUT), a, p, lane, pre, buf, vs);
}

// Channel sums of a register-resident activation tile set (the global-average branch of the NEXT VortexPooling,
// model.py:107-112): x[m][S] of lane (pixel i16, g) holds channels 16S+4g..+3 of pixel p[m].  Within a block the sum
// is formed in fp32 in a fixed order (butterfly over the 16 pixels of a tile, tiles, then the four waves through LDS);
// across blocks it is accumulated as 2^-20 fixed point in int64 (associative: the result does not depend on the
// arrival order, like the integrate kernels' sums) with atomics spread over kColShards rows, so that the block which
// folds the branch into the final convolution's bias (gave_bias_block) reads 16 x 128 words instead of one row per
// block (1200 rows took one block 25 us).  A non-finite block sum sets the channel's flag instead: its mean is NaN,
// as the reference's would be.
constexpr int kColShards = 16;
constexpr float kColScale = 1048576.0f;  // 2^20; |block sum| <= 64 * 65504 -> 4.4e12, 1200 blocks: far inside int64

constexpr int kColMax = 256;  // channels (round 6: the 228-channel entry of the two-head net's last VortexPooling)
struct ColSums {
    long long fix[kColShards][kColMax];
    unsigned bad[kColMax];
};
static_assert(sizeof(ColSums) == kColShards * kColMax * 8 + kColMax * 4, "the layout include/ojf.h gives for ojf_pool_pyramid");
constexpr int colsum_row(int nt) { return nt > 8 ? 256 : 128; }  // floats per wave row of block_colsum's LDS scratch

// v of the lane CTRL names within this lane's row of 16 (a DPP move: VALU, where __shfl_xor goes through the LDS crossbar)
template <int CTRL>
__device__ __forceinline__ float row_dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// DPP: the butterfly's partners come by DPP moves instead of __shfl_xor - the same sums in the same order.  Lane i adds the value of lane
// i ^ 8 (row_ror:8), then of lane (i + 4) & 15 (row_ror:4: that is lane i ^ 4 or lane i ^ 4 ^ 8, which hold the same bits after the first
// step, fp32 addition being commutative), then of lanes i ^ 2 and i ^ 1 (quad_perm).  Only the payload of a NaN can differ, and a
// non-finite sum sets the channel's flag whatever its bits.
template <int MT, int NT, bool DPP = false, int NA = 0>
__device__ __forceinline__ void block_colsum(const f32x4 (&x)[MT][NA], const int (&p)[MT], int npix, float *red /* LDS [waves][colsum_row(NT)] */,
                                             ColSums *out, int lane, int wave, int off = 0)
{
    constexpr int RS = colsum_row(NT);
    const int g = lane >> 4;
#pragma unroll
    for (int S = 0; S < NT; ++S) {
        f32x4 s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < MT; ++m)
            if (p[m] < npix) s += x[m][S];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = s[j];
            if constexpr (DPP) {
                v += row_dpp<0x128>(v);  // row_ror:8
                v += row_dpp<0x124>(v);  // row_ror:4
                v += row_dpp<0x4e>(v);   // quad_perm:[2,3,0,1]
                v += row_dpp<0xb1>(v);   // quad_perm:[1,0,3,2]
            } else {
                v += __shfl_xor(v, 8, 64);
                v += __shfl_xor(v, 4, 64);
                v += __shfl_xor(v, 2, 64);
                v += __shfl_xor(v, 1, 64);
            }
            s[j] = v;
        }
        if ((lane & 15) == 0) *reinterpret_cast<f32x4 *>(red + wave * RS + S * 16 + 4 * g) = s;
    }
    __syncthreads();
    static_assert(NT * 16 <= kChainThreads && NT * 16 <= kColMax, "one thread per channel");
    if ((int)threadIdx.x < NT * 16) {
        const int t = threadIdx.x;
        float v = (red[t] + red[RS + t]) + (red[2 * RS + t] + red[3 * RS + t]);
#pragma unroll
        for (int w4 = 4; w4 < kChainWaves; w4 += 4)  // further waves of the block, four at a time in the same fixed order
            v += (red[w4 * RS + t] + red[(w4 + 1) * RS + t]) + (red[(w4 + 2) * RS + t] + red[(w4 + 3) * RS + t]);
        if (v - v == 0.0f) {  // finite
            const long long q = (long long)__builtin_rintf(v * kColScale);  // |v| < 2^23: the product is exact up to the rounding of rintf
            if (q) atomicAdd(reinterpret_cast<unsigned long long *>(&out->fix[blockIdx.x % kColShards][t + off]), (unsigned long long)q);
        } else {
            atomicOr(&out->bad[t + off], 1u);
        }
    }
}

// Branch-entry GEMM of a VortexPooling (the four branches' first 1x1 convolutions stacked: c_in -> 4 slots of cs
// channels; branch 0 gets bias + ReLU, the pooled branches stay linear) as ONE chain layer on register-resident
// input, plus the per-block channel sums of that input.  Stand-alone form: input = activation planes.  The generic
// convolution kernel needed 25 us for this launch (tap table, masks, 6 output tiles per wave) and a separate
// column-sum launch re-read the same 37 MB.
template <int ARITH, int MT, int NTIN, int NTOUT>
__global__ __launch_bounds__(kChainThreads, kChainBlocks) void entry1x1_kernel(const ChainArgs a)
{
    __shared__ f32x4 wlds[chain_dma(ARITH) ? 2 * kChainDmaHalf : kChainLdsFloat4];
    __shared__ f32x4 vec_lds[2 * kVecF4];
    __shared__ float red[kChainWaves * colsum_row(NTIN)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int strip = (banded_block_x() * kChainWaves + wave) * (MT * 16);
    ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 7, 0);
    ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 0, 0);
    ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 9, banded_block_x() + 1);
    f32x4 pre[kChainPre];
    int buf = 0;
    VecStage vs;
    vs.lds = vec_lds; vs.half = 0;
    {
        VecNext nx;
        nx.a = a.bias; nx.na = chain_bias_stride(ARITH, NTOUT) / 4;
        vec_issue(vs, nx);
    }
    {
        constexpr int size0 = chain_first_size(ARITH, NTIN, NTOUT);
        if constexpr (chain_dma(ARITH)) {
            dma_part(a.w, wlds, size0, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane);
        } else {
#pragma unroll
            for (int k = 0; k < kChainPre; ++k)
                if ((int)threadIdx.x + kChainThreads * k < size0) pre[k] = a.w[threadIdx.x + kChainThreads * k];
        }
    }
    int p[MT];
    f32x4 x[MT][NTIN], y[MT][NTOUT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        p[m] = strip + m * 16 + i16;  // waves past the image still take part in the barriers
#pragma unroll
        for (int S = 0; S < NTIN; ++S) {
            const int G = 4 * S + g;
            const bool ok = p[m] < a.npix && G < a.c4_in;
            x[m][S] = a.in[ok ? (a.in_g0 + G) * a.npix + p[m] : -1];
            if (a.in_split) x[m][S] = unsplit4(x[m][S]);  // hi + lo: exact in fp32, the value every consumer of the halves means
        }
    }
    ENTRY_STAMP_LANDED();
    ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 1, 0);
    if (a.colsum) block_colsum<MT, NTIN>(x, p, a.npix, red, a.colsum, lane, wave);
    ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 2, 0);
    chain_layer<ARITH, MT, NTIN, NTOUT, kChainEntry, 0>(x, y, wlds, a.w, a, p, lane, pre, buf, vs);
}

// Persistent form of the stand-alone entry GEMM for the case the headline net runs (split-fp16, 8 input tiles -> 5, one pixel
// tile per wave).  The one-strip kernel above runs its phases in series - planes in (cold: ~3.9 us of a block's 10), channel
// sums, weight part 0, MFMAs, part 1, MFMAs, stores - and every block streams the layer's 40 KB of weights for its 64 pixels.
// Here a grid of at most kChainBlocks blocks per CU keeps the whole layer and its epilogue vectors in LDS and walks its strips
// (entry_walk_strip: a static assignment - no inter-block wait, flag or ticket, nothing depends on residency); while strip k
// computes, the eight plane loads of strip k + 1 are in flight into a second register set.  The arithmetic of a strip is the
// one-strip kernel's, operation for operation: unsplit4, block_colsum over the same 64 pixels, split_f16 once, each
// accumulator's K blocks ascending in mfma_f16x3's term order, the kChainEntry epilogue - the same bits in the output planes
// and the same integers in ColSums (which fix[] shard a strip adds into differs; the fold sums the shards as integers).
//
// Strip k of block b's walk, -1 past its end.  strips and grid both multiples of 8: block b stays inside XCD band b & 7 (the
// eighth of the strips the one-strip grid gives that XCD) and walks (b >> 3) + k * grid / 8 within it; otherwise b + k * grid.
// (tests/test_entry_gemm_host.py restates it.)
__host__ __device__ __forceinline__ int entry_walk_strip(int b, int grid, int strips, int k)
{
    if (((strips | grid) & 7) == 0) {
        const int per = strips >> 3, j = (b >> 3) + k * (grid >> 3);
        return j < per ? (b & 7) * per + j : -1;
    }
    const int s = b + k * grid;
    return s < strips ? s : -1;
}

// the eight plane loads of one wave's 16 pixels of strip s (s < 0: no such strip - every lane reads the zero float4 in front of the planes)
__device__ __forceinline__ void entry_load_planes(f32x4 (&x)[8], const ChainArgs &a, int s, int wave, int i16, int g)
{
    const int p = (s * kChainWaves + wave) * 16 + i16;
#pragma unroll
    for (int S = 0; S < 8; ++S) {
        const int G = 4 * S + g;
        const bool ok = s >= 0 && p < a.npix && G < a.c4_in;
        x[S] = a.in[ok ? (a.in_g0 + G) * a.npix + p : -1];
    }
}

// dma_part of a compile-time size that gives every wave the same number of 1 KB chunks: no branch around the instructions, so the
// compiler's own waits can count them
template <int SIZE>
__device__ __forceinline__ void entry_dma(const f32x4 *src, f32x4 *dst, int wave, int lane)
{
    static_assert(SIZE % (64 * kChainWaves) == 0, "whole rounds of the block's waves");
#pragma unroll
    for (int c0 = 0; c0 < SIZE / 64; c0 += kChainWaves)
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)(src + (c0 + wave) * 64 + lane),
                                         (void __attribute__((address_space(3))) *)(dst + (c0 + wave) * 64), 16, 0, 0);
}

// MFMAs of CNT output tiles (accumulators y[NB ..]) over the KB K blocks, weights at wpart [tile][K block][hi 64 | lo 64]: K block
// outer, tile inner, fragments requested kChainAhead steps ahead of their MFMAs (chain_layer's pipeline)
template <int KB, int NB, int CNT, int NY>
__device__ __forceinline__ void entry_mfma_tiles(const f32x4 *wpart, int lane, const f16x8 (&xh)[KB], const f16x8 (&xl)[KB], f32x4 (&y)[NY])
{
    constexpr int steps = KB * CNT;
    f32x4 rh[kChainAhead], rl[kChainAhead];
    auto frag = [&](int t) { return ((t % CNT) * KB + t / CNT) * 128; };  // step t = (S = t / CNT, tile NB + t % CNT)
#pragma unroll
    for (int t = 0; t < kChainAhead; ++t) {
        rh[t] = wpart[frag(t) + lane];
        rl[t] = wpart[frag(t) + 64 + lane];
    }
#pragma unroll
    for (int t = 0; t < steps; ++t) {
        const f32x4 wh = rh[t % kChainAhead], wl = rl[t % kChainAhead];
        if (t + kChainAhead < steps) {
            rh[t % kChainAhead] = wpart[frag(t + kChainAhead) + lane];
            rl[t % kChainAhead] = wpart[frag(t + kChainAhead) + 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);
        y[NB + t % CNT] = mfma_f16x3(wh, wl, xh[t / CNT], xl[t / CNT], y[NB + t % CNT]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <bool IN_SPLIT>  // the input planes are split planes (the dense-growth buffer of dense_chain_kernel: the headline) | plain fp32
__global__ __launch_bounds__(kChainThreads, kChainBlocks) void entry1x1_persistent_kernel(const ChainArgs a, const int strips)
{
    constexpr int ARITH = OJF_ARITH_F16X3, NTIN = 8, NTOUT = 5, KB = chain_kblocks(ARITH, NTIN);
    constexpr int kSize = chain_layer_size(ARITH, NTIN, NTOUT);  // 2560 float4
    constexpr int kVec = chain_bias_stride(ARITH, NTOUT) / 4;
    static_assert(kVec <= kVecF4 && kVec <= kChainThreads, "one float4 of the epilogue vectors per thread");
    __shared__ f32x4 wlds[kSize];
    __shared__ f32x4 vec[kVecF4];
    // two rows: the readers of strip k's partial sums and the writers of strip k + 1's are separated by no barrier, those of strip k + 2's
    // by the barrier inside strip k + 1's block_colsum
    __shared__ float red[2][kChainWaves * colsum_row(NTIN)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int s = entry_walk_strip(blockIdx.x, gridDim.x, strips, 0);
    ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 7, 0);
    ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 0, 0);
    // Vector-memory order of a wave: epilogue vectors | the layer's weights (10 DMA instructions) | planes of the first strip || planes
    // of the second strip.  Loads complete in order, and the first strip's planes - cold, written by dense_chain_kernel on other XCDs -
    // are the last to land: one wait covers all three, and the weights cost a block nothing beyond the plane latency it pays anyway.
    // (Two DMA groups with waits of their own, as in the one-strip kernel, do not survive the compiler here: while a DMA instruction
    // is in flight in its model it puts a full vmcnt wait in front of the next LDS read, LDS write and __syncthreads - with tiles 3..4
    // requested behind the first barrier the first MFMAs waited for them all the same, and with them requested behind the first strip's
    // planes the channel sums' barrier waited for the second strip's planes.)
    f32x4 vreg = f32x4{0.f, 0.f, 0.f, 0.f};
    if ((int)threadIdx.x < kVec) vreg = reinterpret_cast<const f32x4 *>(a.bias)[threadIdx.x];
    entry_dma<kSize>(a.w, wlds, wave_u, lane);
    f32x4 xn[NTIN], x[1][NTIN];
    entry_load_planes(xn, a, s, wave, i16, g);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's chunks of the weights and its planes have landed
    ENTRY_STAMP(ENTRY_STAMP_ON(a), 0, 1, 0);
    if ((int)threadIdx.x < kVec) vec[threadIdx.x] = vreg;  // published by the first barrier of the loop
#pragma unroll
    for (int S = 0; S < NTIN; ++S) x[0][S] = IN_SPLIT ? unsplit4(xn[S]) : xn[S];  // hi + lo: exact in fp32, the value every consumer of the halves means
    int sn = entry_walk_strip(blockIdx.x, gridDim.x, strips, 1);
    entry_load_planes(xn, a, sn, wave, i16, g);  // in flight while the first strip computes
    asm volatile("" ::: "memory");
    float gmax = 0.0f;
    for (int k = 0; s >= 0; ++k) {
        ENTRY_STAMP(ENTRY_STAMP_ON(a), k, 9, s + 1);
        // (opaque copy of the lane's channel-group index: left alone, the compiler hoists every mask and address part derived from it out of the
        // loop - 38 lane masks and 13 address pairs held across the strips, which spilled both register files)
        int gk = g;
        asm volatile("" : "+v"(gk));
        const int p[1] = {(s * kChainWaves + wave) * 16 + i16};  // waves past the image still take part in the barriers
        // (the butterfly by DPP moves: 128 ds_bpermute per wave and strip through the LDS crossbar were 1.8 us of a strip's 5.4)
        if (a.colsum) block_colsum<1, NTIN, true>(x, p, a.npix, red[k & 1], a.colsum, lane, wave);
        ENTRY_STAMP(ENTRY_STAMP_ON(a), k, 2, 0);
        f16x8 xh[KB], xl[KB];
#pragma unroll
        for (int S = 0; S < KB; ++S) split_f16(x[0][2 * S], x[0][2 * S + 1], xh[S], xl[S]);
        f32x4 y[NTOUT];
#pragma unroll
        for (int n2 = 0; n2 < NTOUT; ++n2) y[n2] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k == 0) {  // the weights: every wave waited for its chunks above
            __syncthreads();
            ENTRY_STAMP(ENTRY_STAMP_ON(a), k, 3, 0);
        }
        // one round over the five tiles where the one-strip kernel runs tiles 0..2, then 3..4: each accumulator still takes its K blocks in
        // ascending order, and nothing else decides its bits
        entry_mfma_tiles<KB, 0, NTOUT>(wlds, lane, xh, xl, y);
        ENTRY_STAMP(ENTRY_STAMP_ON(a), k, 5, 0);
        // The next strip's planes, requested one strip ago, leave their registers BEFORE this strip's stores are issued: stores count in
        // vmcnt like loads, so a wait for the planes at the top of the next strip would also wait for the stores' acknowledgements.
        const int s_next = sn;
        if (s_next >= 0) {
#pragma unroll
            for (int S = 0; S < NTIN; ++S) x[0][S] = IN_SPLIT ? unsplit4(xn[S]) : xn[S];
#ifdef OJF_ENTRY_STAMPS
            __builtin_amdgcn_sched_barrier(0);  // (the stamp stays behind the wait the conversions needed)
            ENTRY_STAMP(ENTRY_STAMP_ON(a), k + 1, 1, 0);
#endif
            sn = entry_walk_strip(blockIdx.x, gridDim.x, strips, k + 2);
            entry_load_planes(xn, a, sn, wave, i16, gk);
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int n2 = 0; n2 < NTOUT; ++n2) {  // chain_layer's kChainEntry epilogue
            const int og = n2 * 4 + gk;
            const f32x4 lin4 = fma4(y[n2], vec[(NTOUT + n2) * 4 + g], vec[n2 * 4 + g]);
            f32x4 v = lin4;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (og * 4 + j < a.act_n && !(v[j] > 0.0f)) ? (v[j] != v[j] ? v[j] : 0.0f) : v[j];
            if (p[0] < a.npix && og < a.og_store) {
                a.out_planes[(size_t)(a.out_g0 + og) * a.npix + p[0]] = og < a.split_groups ? split_pack4(v) : v;
                gmax = guard_max(gmax, lin4);  // over stored elements only
            }
        }
        ENTRY_STAMP(ENTRY_STAMP_ON(a), k, 6, 0);
        ENTRY_STAMP(ENTRY_STAMP_ON(a), k, 8, 0);
        s = s_next;
        ENTRY_STAMP(ENTRY_STAMP_ON(a) && s >= 0, k + 1, 7, 0);
        ENTRY_STAMP(ENTRY_STAMP_ON(a) && s >= 0, k + 1, 0, 0);
    }
    if (gmax > 65504.0f && a.ovf) guard_raise(a.ovf, 1);
}

// ------------------------------------------------------------------------------------------------
// Fused VortexPooling tail (model.py:131-141,157-159): for each of the four branches
//   t_b = ReLU(W1_b v_b + b1_b)   (mid -> out channels, the branch's closing 1x1 + BN + ReLU)
//   y  += Wf_b t_b                (that branch's column block of the final 1x1 over the concat)
// followed by y + bias' (final conv bias + BN + the folded global-average branch).  The 4 x 116-channel
// concat tensor of the reference never exists: t_b lives in registers between the two GEMMs (same
// accumulator -> operand identity as the prediction-head chain) and y accumulates across branches.
// ------------------------------------------------------------------------------------------------
struct TailArgs {
    const f32x4 *v[4];  // branch inputs (planes, c4 groups each)
    const f32x4 *w;     // stream: W1_0 [NO][NV], Wf_0 [NO][NO], W1_1, Wf_1, ... (chain_layer fragments)
    const float *b1;    // 4 x chain_bias_stride: closing-1x1 biases (+ inverse row scales)
    const float *bias_final;  // NO*16 (per-frame: includes the global-average branch)
    const float *rinv_final;  // split-fp16: NO*16 inverse row scales of the final conv (common to the four blocks)
    f32x4 *out;
    int c4, out_g0, og_store, npix;
    int *ovf;  // split-fp16 range guard flag (see ConvArgs)
    // CHAIN variants (the last VortexPooling of the net): the prediction head runs on the register-resident result
    const f32x4 *chain_w;
    const float *chain_b;
    float *out_rows;
    int rows_stride, rows_n;
    float scale;
    // CHAIN = kTailEntry (a VortexPooling that feeds the next one): the next branch-entry GEMM runs on the register-
    // resident result, which is never written: planes of 4*cs channels + per-block channel sums come out instead
    const f32x4 *entry_w;
    const float *entry_b;
    f32x4 *entry_out;
    int entry_og, entry_act_n;
    struct ColSums *colsum;
    int entry_split;  // ChainArgs::split_groups of the fused entry layer
    int colsum_off = 0;  // two-head nets: this head's channels start here in the next VortexPooling's input (hd * os)
};

constexpr int kTailEntry = 1;

// the prediction-head topologies chain_run is instantiated for (growth channels 19 / 20)
template <int ARITH, int MT, int KIND>
__device__ __forceinline__ void head_run(f32x4 (&x)[MT][8], f32x4 (&y)[MT][8], f32x4 *wlds, const f32x4 *wg, const float *bias,
                                         const ChainArgs &a, const int (&p)[MT], int lane, f32x4 (&pre)[kChainPre], int &buf,
                                         VecStage &vs)
{
    if constexpr (KIND == 19) chain_run<ARITH, MT, 8, 6, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1>(x, y, wlds, wg, bias, a, p, lane, pre, buf, vs);
    else chain_run<ARITH, MT, 8, 7, 7, 5, 5, 4, 4, 3, 3, 2, 2, 1>(x, y, wlds, wg, bias, a, p, lane, pre, buf, vs);
}
constexpr int head_first_ntout(int kind) { return kind == 19 ? 6 : 7; }
constexpr int head_first_size(int arith, int kind) { return chain_first_size(arith, 8, kind == 19 ? 6 : 7); }

// When a block asks for its branch inputs.  They are cold (written by the grouped 3x3 launch just before, on other XCDs), and every
// chain_layer part begins with a full vmcnt wait and a barrier, so a request at a branch's head is a global round trip the block sits
// out at once - four per block.  kTailNext: branch b + 1's planes are requested behind the first barrier of branch b's closing 1x1 and
// land under that branch's parts (8 more VGPRs, still three blocks per CU), and the butterfly of the fused entry layer's channel sums
// runs on DPP moves.  kTailAtBranch: the requests at each branch's head and the __shfl_xor butterfly - the same arithmetic and the same
// bits, kept for ojf_vortex_tail's form 0 (tests) and the profiling build.  Where the time of a block goes in either form, and the form
// with all four branches requested at block start that was not kept: profiles/vortex_tail_block_life.txt.
constexpr int kTailAtBranch = 0, kTailNext = 1;

// the planes of branch b for this wave's pixels (lanes outside the frame or the branch's groups read the zero float4 in front of the planes)
template <int MT, int NV>
__device__ __forceinline__ void tail_load_branch(f32x4 (&vin)[MT][NV], const TailArgs &a, int b, const int (&p)[MT], int g)
{
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int S = 0; S < NV; ++S) {
            const int G = 4 * S + g;
            const bool ok = p[m] < a.npix && G < a.c4;
            vin[m][S] = a.v[b][ok ? G * a.npix + p[m] : -1];
        }
}

// CHAIN = 0: write the VortexPooling result planes.  CHAIN = 19 / 20: feed it straight into the prediction head
// (same accumulator -> operand identity) and write est rows; the 114-channel tensor between them never exists.
template <int ARITH, int MT, int NV, int NO, int CHAIN = 0, int FORM = kTailNext>
__global__ __launch_bounds__(kChainThreads, kChainBlocks) void vortex_tail_kernel(const TailArgs a)
{
    [[maybe_unused]] constexpr int kStampKind = CHAIN > kTailEntry ? 1 : 0;
    TAIL_STAMP(kStampKind, 16, 0);
    TAIL_STAMP(kStampKind, 0, 0);
    TAIL_STAMP(kStampKind, 18, blockIdx.x + 1);
    static_assert(CHAIN == 0 || NO == 8, "the fused prediction head / entry layer expects 8 input tiles");
    __shared__ f32x4 wlds[chain_dma(ARITH) ? 2 * kChainDmaHalf : kChainLdsFloat4];
    __shared__ f32x4 vec_lds[2 * kVecF4];
    __shared__ float red[CHAIN == kTailEntry ? kChainWaves * 128 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int strip = (banded_block_x() * kChainWaves + wave) * (MT * 16);
    int p[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) p[m] = strip + m * 16 + i16;
    // epilogue vectors one layer ahead (VecStage): branch b's closing-1x1 vectors travel during branch b - 1, the final
    // bias / scale during the last branch, the fused entry layer's / head's first vectors during the last accumulation
    constexpr int kVec1 = chain_bias_stride(ARITH, NO) / 4, kVecFin = NO * 4 * (ARITH == OJF_ARITH_F16X3 ? 2 : 1);
    VecStage vs;
    vs.lds = vec_lds; vs.half = 0;
    {
        VecNext nx;
        nx.a = a.b1; nx.na = kVec1;
        vec_issue(vs, nx);
    }
    ChainArgs ca;  // only npix is read by the layer code in these modes
    ca.npix = a.npix; ca.out_rows = nullptr; ca.rows_n = 0; ca.rows_stride = 0; ca.scale = 1.0f; ca.ovf = a.ovf;
    f32x4 y[MT][NO];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NO; ++n) y[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 pre[kChainPre];
    int buf = 0;
    {
        constexpr int size0 = chain_first_size(ARITH, NV, NO);
        if constexpr (chain_dma(ARITH)) {
            dma_part(a.w, wlds, size0, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane);
        } else {
#pragma unroll
            for (int k = 0; k < kChainPre; ++k)
                if ((int)threadIdx.x + kChainThreads * k < size0) pre[k] = a.w[threadIdx.x + kChainThreads * k];
        }
    }
    constexpr size_t per_branch = (size_t)chain_layer_size(ARITH, NV, NO) + chain_layer_size(ARITH, NO, NO);
    f32x4 t[MT][NO];
    const f32x4 *vfin = vec_lds;
    f32x4 vin[4][MT][NV];
    if constexpr (FORM == kTailNext) tail_load_branch(vin[0], a, 0, p, g);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        if constexpr (FORM == kTailAtBranch) tail_load_branch(vin[b], a, b, p, g);
        TAIL_STAMP_LANDED();
        TAIL_STAMP(kStampKind, 1 + 3 * b, 0);
        const f32x4 *w1 = a.w + b * per_branch, *wf = w1 + (size_t)chain_layer_size(ARITH, NV, NO);
        VecNext nx;  // what travels during this branch's closing 1x1
        if (b < 3) {
            nx.a = a.b1 + (b + 1) * chain_bias_stride(ARITH, NO); nx.na = kVec1;
        } else {
            nx.a = a.bias_final; nx.na = NO * 4;
            if constexpr (ARITH == OJF_ARITH_F16X3) { nx.b = a.rinv_final; nx.nb = NO * 4; }
        }
        // kTailNext: the next branch's planes are requested behind this layer's first barrier (chain_layer's hook); none after the last
        constexpr int kLast = 3;
        const int bn = b < kLast ? b + 1 : kLast;
        auto next_planes = [&]() {
            if (FORM == kTailNext && b < kLast) tail_load_branch(vin[bn], a, bn, p, g);
        };
        chain_layer<ARITH, MT, NV, NO, kChainRelu, chain_first_size(ARITH, NO, NO)>(vin[b], t, wlds, w1, ca, p, lane, pre, buf, vs, nx,
                                                                                    nullptr, 0, next_planes);
        TAIL_STAMP(kStampKind, 2 + 3 * b, 0);
        if (b < 3) {
            chain_layer<ARITH, MT, NO, NO, kChainAccumulate, chain_first_size(ARITH, NV, NO)>(t, y, wlds, wf, ca, p, lane, pre, buf, vs);
        } else {
            vfin = vs.lds + vs.half * kVecF4;  // the half the last accumulation commits the final vectors to
            VecNext nf;
            if constexpr (CHAIN == kTailEntry) { nf.a = a.entry_b; nf.na = chain_bias_stride(ARITH, 5) / 4; }
            else if constexpr (CHAIN != 0) { nf.a = a.chain_b; nf.na = chain_bias_stride(ARITH, head_first_ntout(CHAIN)) / 4; }
            chain_layer<ARITH, MT, NO, NO, kChainAccumulate,
                        CHAIN == kTailEntry ? chain_first_size(ARITH, 8, 5) : (CHAIN ? head_first_size(ARITH, CHAIN) : 0)>(
                t, y, wlds, wf, ca, p, lane, pre, buf, vs, nf, CHAIN == kTailEntry ? a.entry_w : a.chain_w, kVecFin);
        }
        TAIL_STAMP(kStampKind, 3 + 3 * b, 0);
    }
    float gmax = 0.0f;
#pragma unroll
    for (int n = 0; n < NO; ++n) {
        const int og = n * 4 + g;
        const f32x4 bf = vfin[n * 4 + g];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            f32x4 v = y[m][n] + bf;
            if constexpr (ARITH == OJF_ARITH_F16X3) v = fma4(y[m][n], vfin[NO * 4 + n * 4 + g], bf);
            if constexpr (ARITH == OJF_ARITH_F16X3) gmax = guard_max(gmax, v);
            if constexpr (CHAIN) y[m][n] = v;
            else if (p[m] < a.npix && og < a.og_store) a.out[(size_t)(a.out_g0 + og) * a.npix + p[m]] = v;
        }
    }
    if constexpr (ARITH == OJF_ARITH_F16X3)
        if (gmax > 65504.0f && a.ovf) guard_raise(a.ovf, 1);
    TAIL_STAMP(kStampKind, 13, 0);
    if constexpr (CHAIN == kTailEntry) {
        // (the butterfly by DPP moves: 128 ds_bpermute per wave through the LDS crossbar otherwise, see entry1x1_persistent_kernel)
        block_colsum<MT, NO, FORM != kTailAtBranch>(y, p, a.npix, red, a.colsum, lane, wave, a.colsum_off);
        TAIL_STAMP(kStampKind, 14, 0);
        ca.out_planes = a.entry_out; ca.out_g0 = 0; ca.og_store = a.entry_og; ca.act_n = a.entry_act_n; ca.split_groups = a.entry_split;
        chain_layer<ARITH, MT, 8, 5, kChainEntry, 0>(y, t, wlds, a.entry_w, ca, p, lane, pre, buf, vs);
    } else if constexpr (CHAIN) {
        ca.out_rows = a.out_rows; ca.rows_stride = a.rows_stride; ca.rows_n = a.rows_n; ca.scale = a.scale;
        head_run<ARITH, MT, CHAIN>(y, t, wlds, a.chain_w, a.chain_b, ca, p, lane, pre, buf, vs);
    }
    TAIL_STAMP(kStampKind, 15, 0);
    TAIL_STAMP(kStampKind, 17, 0);
}

// Pool pyramid of a VortexPooling (model.py:143-155): branch b = 1..3 sees its entry-conv pre-activation pooled b
// times by nn.AvgPool2d(3, 1, 1) (zero padding, count_include_pad: always / 9), then bias + ReLU.  One launch:
// a block takes a 32x8-pixel tile of ONE channel group, stages it with a halo of b pixels in LDS and applies the b
// pooling levels there (every level is zero outside the image, like the padded intermediate tensors of the
// reference); the intermediate levels never reach HBM.  Summation order per level = row-major taps, as before, then one
// correctly rounded division by 9 (div9).  Where the launch's time goes: profiles/pool_pyramid_launch.txt.
// (used by gave_bias_block below; declared here because the pyramid launch carries one)
struct GaveArgs {
    const float *partial;   // general flow: nparts rows of pstride floats, added in row order
    struct ColSums *fixed;  // chain flow: fixed-point sums (read, then zeroed for the next frame)
    int nparts, pstride, cphys, npix;
    const float *WgT, *bg, *WfgT, *bf;  // WgT [cphys][c_out], WfgT [c_out(j)][c_out(o)]: lane o reads consecutive addresses
    int c_out;
    float *bias_out;
    int bias_len;
};

struct PyramidArgs {
    const f32x4 *z;        // entry-conv output planes; branch b's pre-activation = groups [b*c4, (b+1)*c4)
    f32x4 *q[3];           // branch inputs out: planes of c4 groups each
    const float *bias[3];  // per branch: c4*4 floats
    int h, w, c4;
    int tiles;      // pixel tiles; with fold_gave, block column `tiles` folds the global-average branch instead
    int fold_gave;
    // two-head nets: the entry GEMM arrives as two partial sums (one per head, no bias, no activation): z + z2 on load; block rows
    // [3 c4, 4 c4) form branch 0 = ReLU(z + z2 + bias0) (no pooling) into q0
    const f32x4 *z2 = nullptr;
    f32x4 *q0 = nullptr;
    const float *bias0 = nullptr;
    int split_out;  // q[] are split planes (split_pack4): their only reader is the branch's first 3x3 convolution
    GaveArgs gave;
};

constexpr int kPoolTW = 32, kPoolTH = 8, kPoolStride = kPoolTW + 6;
constexpr int kPoolPH = 2;  // outputs per thread and level, a column (4: 82 VGPRs, five blocks per CU instead of eight)
static_assert((kPoolTW + 4) * ((kPoolTH + 4 + kPoolPH - 1) / kPoolPH) <= 256, "one pass of the block covers the widest level");

// x / 9.0f, correctly rounded, in five instructions instead of the compiler's division sequence (scale, reciprocal, four fused steps,
// fix-up: the divisions were a quarter of the pooling blocks' run time): q = RN(x * RN(1/9)) is within an ulp, the residual x - 9 q is
// exact in one fma, and q + residual * RN(1/9) rounds to RN(x / 9).  Compared with x / 9.0f over ALL 2^32 bit patterns on the host
// (denormals included): equal bit for bit except for -0 and the infinities, where q == x (and only there) - those return x.  NaN stays NaN.
__device__ __forceinline__ float div9(float x)
{
    const float r = 1.0f / 9.0f;
    const float q = x * r;
    const float f = __builtin_fmaf(__builtin_fmaf(-9.0f, q, x), r, q);
    return q == x ? x : f;
}

// LV = pooling levels of this block's channel group: region sizes are compile-time (the per-element index
// divisions become multiplies)
template <int LV>
__device__ __forceinline__ void pool_pyramid_body(const PyramidArgs &a, f32x4 (&buf)[2][kPoolStride * (kPoolTH + 6)], int cg)
{
    const int tiles_x = (a.w + kPoolTW - 1) / kPoolTW;
    const int tile = banded_block_x();
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * kPoolTW, y0 = ty * kPoolTH, npix = a.h * a.w;
    const f32x4 *plane = a.z + (size_t)(LV * a.c4 + cg) * npix;
    const f32x4 *plane2 = a.z2 ? a.z2 + (size_t)(LV * a.c4 + cg) * npix : nullptr;  // (uniform)
    const f32x4 zero{0.f, 0.f, 0.f, 0.f};
    {   // the tile with its halo: every load is requested before the first one is waited for
        constexpr int W0 = kPoolTW + 2 * LV, H0 = kPoolTH + 2 * LV, N0 = (W0 * H0 + 255) / 256;
        f32x4 v[N0];
        int at[N0];  // pixel, -1 outside the image (or past the region)
#pragma unroll
        for (int k = 0; k < N0; ++k) {
            const int i = k * 256 + threadIdx.x;
            const int ly = i / W0, lx = i - ly * W0;
            const int gy = y0 - LV + ly, gx = x0 - LV + lx;
            const bool in = i < W0 * H0 && (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
            at[k] = in ? gy * a.w + gx : -1;
            v[k] = in ? plane[at[k]] : zero;
        }
        if (plane2) {
#pragma unroll
            for (int k = 0; k < N0; ++k)
                if (at[k] >= 0) v[k] += plane2[at[k]];
        }
#pragma unroll
        for (int k = 0; k < N0; ++k) {
            const int i = k * 256 + threadIdx.x;
            const int ly = i / W0, lx = i - ly * W0;
            if (i < W0 * H0) buf[0][ly * kPoolStride + lx] = v[k];
        }
    }
    __syncthreads();
    // A thread forms a column of kPoolPH outputs of a level from registers: the kPoolPH + 2 source rows of three values each are read once
    // (3 (PH + 2) / PH LDS reads per output instead of 9) and every output adds its nine taps in row-major order, as before.
#pragma unroll
    for (int l = 1; l <= LV; ++l) {
        const int halo = LV - l;  // halo of this level's region; the source region has halo + 1
        const int Wl = kPoolTW + 2 * halo, Hl = kPoolTH + 2 * halo, NP = (Hl + kPoolPH - 1) / kPoolPH;
        const bool whole = Hl % kPoolPH == 0;  // no ragged last patch
        const f32x4 *src = buf[(l - 1) & 1];
        const int i = threadIdx.x;
        if (i < Wl * NP) {
            const int pr = i / Wl, lx = i - pr * Wl, ly0 = pr * kPoolPH;
            f32x4 acc[kPoolPH];
#pragma unroll
            for (int o = 0; o < kPoolPH; ++o) acc[o] = zero;
#pragma unroll
            for (int r = 0; r < kPoolPH + 2; ++r) {
                if (whole || ly0 + r < Hl + 2) {
                    const f32x4 *row = src + (ly0 + r) * kPoolStride + lx;
                    const f32x4 t0 = row[0], t1 = row[1], t2 = row[2];
#pragma unroll
                    for (int o = 0; o < kPoolPH; ++o)
                        if (r - o >= 0 && r - o <= 2) {  // tap row r - o of output o
                            acc[o] += t0;
                            acc[o] += t1;
                            acc[o] += t2;
                        }
                }
            }
            const int gx = x0 - halo + lx;
#pragma unroll
            for (int o = 0; o < kPoolPH; ++o) {
                const int ly = ly0 + o, gy = y0 - halo + ly;
                if (!whole && ly >= Hl) break;
                const bool in = (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
                f32x4 s;
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] = div9(acc[o][j]);
                if (l < LV) {
                    buf[l & 1][ly * kPoolStride + lx] = in ? s : zero;
                } else if (in) {
                    s += *reinterpret_cast<const f32x4 *>(a.bias[LV - 1] + 4 * cg);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[j] = s[j] < 0.0f ? 0.0f : s[j];  // keeps NaN, like torch.relu
                    a.q[LV - 1][(size_t)cg * npix + gy * a.w + gx] = a.split_out ? split_pack4(s) : s;
                }
            }
        }
        if (l < LV) __syncthreads();
    }
}

constexpr int kGaveLds = 128 + 256 * 3;  // float4 of LDS gave_bias_block works in
__device__ __forceinline__ void gave_bias_block(const GaveArgs &a, float *lds);

#ifdef OJF_POOL_STAMPS  // profiling build only (tools/pool_stamps.py): wall-clock stamps (100 MHz) of every block's start and end, thread 0
constexpr int kPoolStampBlocks = 8192;
__device__ unsigned long long g_pool_stamps[kPoolStampBlocks][2];
#define POOL_STAMP(i) do { const unsigned b_ = blockIdx.y * gridDim.x + blockIdx.x; if (threadIdx.x == 0 && b_ < (unsigned)kPoolStampBlocks - 8) g_pool_stamps[b_][i] = wall_clock64(); } while (0)
// phases of the block that folds the global-average branch, in the last eight rows: 0 start, 1 mean formed, 2 first mat-vec done, 3 end
#define FOLD_STAMP(i) do { if (threadIdx.x == 0) g_pool_stamps[kPoolStampBlocks - 8 + (i)][0] = wall_clock64(); } while (0)
#else
#define POOL_STAMP(i) do { } while (0)
#define FOLD_STAMP(i) do { } while (0)
#endif

__device__ __forceinline__ void pool_pyramid_block(const PyramidArgs &a, f32x4 (&buf)[2][kPoolStride * (kPoolTH + 6)])
{
    static_assert(2 * kPoolStride * (kPoolTH + 6) >= kGaveLds, "the fold block works in the pools' LDS");
    if (banded_block_x() >= a.tiles) {  // one of the padding blocks: the global-average branch -> bias of the final conv
        // (it starts with the launch and has to end before the pools do: its weights stream in, see gave_bias_block)
        if (blockIdx.y == 0 && banded_block_x() == a.tiles && a.fold_gave) gave_bias_block(a.gave, reinterpret_cast<float *>(buf));
        return;
    }
    // levels of this block's group.  The groups are dispatched in blockIdx.y order: the three-level blocks (three cascaded pools from one
    // window) first, the one-level blocks and the two-head nets' pool-free row last, so that the launch ends on its cheap blocks
    const int yg = blockIdx.y / a.c4, cg = blockIdx.y - yg * a.c4;
    const int lv = yg < 3 ? 3 - yg : 4;
    if (lv == 4) {  // two-head nets: branch 0 of the VortexPooling = ReLU(sum of the two heads' partial entry sums + bias), no pooling
        const int tiles_x = (a.w + kPoolTW - 1) / kPoolTW;
        const int tile = banded_block_x();
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int gy = ty * kPoolTH + (int)threadIdx.x / kPoolTW, gx = tx * kPoolTW + (int)threadIdx.x % kPoolTW;
        if (gy < a.h && gx < a.w) {
            const size_t at = (size_t)cg * a.h * a.w + gy * a.w + gx;
            f32x4 v = a.z[at] + a.z2[at] + *reinterpret_cast<const f32x4 *>(a.bias0 + 4 * cg);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] < 0.0f ? 0.0f : v[j];  // keeps NaN, like torch.relu
            a.q0[at] = a.split_out ? split_pack4(v) : v;
        }
        return;
    }
    if (lv == 1) pool_pyramid_body<1>(a, buf, cg);
    else if (lv == 2) pool_pyramid_body<2>(a, buf, cg);
    else pool_pyramid_body<3>(a, buf, cg);
}

__global__ __launch_bounds__(256) void pool_pyramid_kernel(const PyramidArgs a)
{
    __shared__ f32x4 buf[2][kPoolStride * (kPoolTH + 6)];
    POOL_STAMP(0);
    pool_pyramid_block(a, buf);
    POOL_STAMP(1);
}

constexpr int kSumBlocks = 32;

// per-channel partial sums (deterministic two-stage global average): block (b, cg) sums the float4s
// of plane cg over pixel strip b; fixed-order shuffle + LDS reduction
__global__ __launch_bounds__(256) void colsum_kernel(const f32x4 *in, int g0, int npix, float *partial)
{
    __shared__ f32x4 red[4];
    const int cg = blockIdx.y;
    const int per = (npix + gridDim.x - 1) / gridDim.x;
    const int p0 = blockIdx.x * per, p1 = min(npix, p0 + per);
    const f32x4 *plane = in + (size_t)(g0 + cg) * npix;
    f32x4 s{0.f, 0.f, 0.f, 0.f};
    for (int p = p0 + threadIdx.x; p < p1; p += 256) s += plane[p];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_down(s[j], off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = (red[0] + red[1]) + (red[2] + red[3]);
        *reinterpret_cast<f32x4 *>(partial + (size_t)blockIdx.x * 256 + 4 * cg) = s;
    }
}

// gave_pool branch (model.py:107-112) folded into the bias of the final 1x1 conv:
//   mean -> 1x1 conv (+BN folded) -> g[c_out];  bias' = bias_final + W_final[:, gave columns] @ g
// `partial`: nparts rows of pstride floats (per-block channel sums), added in row order.

//
// The two mat-vecs keep one fmaf chain per output (input channels ascending); only the way the weights arrive differs from
// one-load-per-step chains (16 dependent global round trips per mat-vec, 0.5-0.7 us each: the whole pyramid launch waited for
// this block).  No weight address depends on data, so the block streams both matrices, one after the other, as flat 16-byte
// loads of all 256 threads in chunks of kGaveChunk float4: two chunks are in flight in registers from the top of the block
// (before the channel sums come back) while the chains consume the chunk that sits in LDS.
constexpr int kGavePer = 3, kGaveChunk = 256 * kGavePer;  // float4 per thread and per chunk
static_assert(kGaveLds == 128 + kGaveChunk, "float4: mean[256], gv[256], the chunk");

struct GaveStream {
    const float *W[2];  // WgT, WfgT
    int rows[2];        // cphys, c_out
    int chunks[2];
    int c_out, R;       // a chunk = R whole rows (a multiple of 4: every chunk starts on a float4), R * c_out <= 4 * kGaveChunk floats
};

// Every load is unconditional (addresses clamped into the matrix, chunks past the end fetch the last one again): with loads
// under branches the compiler waits for ALL loads in flight before it writes a chunk to LDS, the younger chunk's included, and
// the stream is one round trip per chunk again.
__device__ __forceinline__ void gave_fetch(const GaveStream &gs, int g, f32x4 (&r)[kGavePer])
{
    g = min(g, gs.chunks[0] + gs.chunks[1] - 1);
    const int m = g < gs.chunks[0] ? 0 : 1, k = m ? g - gs.chunks[0] : g;
    const int f0 = k * gs.R * gs.c_out, last = (gs.rows[m] * gs.c_out - 1) & ~3;  // the matrix's last float4 (its allocation is rounded up)
    const float *W = gs.W[m];
#pragma unroll
    for (int i = 0; i < kGavePer; ++i) r[i] = *reinterpret_cast<const f32x4 *>(W + min(f0 + 4 * (i * 256 + (int)threadIdx.x), last));
}

// chunk g: registers -> LDS, the registers take chunk g + 2, the chains advance over the rows of the chunk
__device__ __forceinline__ void gave_step(const GaveArgs &a, const GaveStream &gs, int g, f32x4 (&r)[kGavePer], f32x4 *stage,
                                          const float *mean, float *gv, float &s, float bf)
{
    const int t = threadIdx.x;
    if (g >= gs.chunks[0] + gs.chunks[1]) return;  // (uniform)
    const int m = g < gs.chunks[0] ? 0 : 1, k = m ? g - gs.chunks[0] : g;
    __syncthreads();  // the chains are done with the previous chunk
#pragma unroll
    for (int i = 0; i < kGavePer; ++i) stage[i * 256 + t] = r[i];
    if (m == 1 && k == 0) {  // first mat-vec complete: its result is the second one's input
        gv[t] = t < a.c_out ? s : 0.0f;
        s = bf;
        FOLD_STAMP(2);
    }
    gave_fetch(gs, g + 2, r);
    __syncthreads();
    if (t < a.c_out) {
        const int n = min(gs.R, gs.rows[m] - k * gs.R);  // (uniform) rows of this chunk
        const float *x = (m ? gv : mean) + k * gs.R, *wl = reinterpret_cast<const float *>(stage) + t;
#pragma unroll 8
        for (int c = 0; c < n; ++c) s = __builtin_fmaf(wl[c * a.c_out], x[c], s);
    }
}

__device__ __forceinline__ void gave_bias_block(const GaveArgs &a, float *lds /* LDS [4 * kGaveLds], 16-byte aligned */)
{
    float *mean = lds, *gv = lds + 256;
    f32x4 *stage = reinterpret_cast<f32x4 *>(lds + 512);
    const int t = threadIdx.x;
    GaveStream gs;
    gs.W[0] = a.WgT; gs.W[1] = a.WfgT;
    gs.rows[0] = a.cphys; gs.rows[1] = a.c_out;
    gs.c_out = a.c_out; gs.R = (4 * kGaveChunk / a.c_out) & ~3;  // c_out <= 256: R >= 12
    for (int m = 0; m < 2; ++m) gs.chunks[m] = (gs.rows[m] + gs.R - 1) / gs.R;
    FOLD_STAMP(0);
    f32x4 r0[kGavePer], r1[kGavePer];
    gave_fetch(gs, 0, r0);
    gave_fetch(gs, 1, r1);
    const float bg = t < a.c_out ? a.bg[t] : 0.0f, bf = t < a.c_out ? a.bf[t] : 0.0f;
    if (a.fixed) {
        // (sixteen shard loads per thread in flight beside the two weight chunks cost the kernel its eight blocks per CU: 82 VGPRs)
        long long *qs = reinterpret_cast<long long *>(stage);  // (free until the first chunk lands)
        static_assert(kColMax == 256, "one thread per channel");
        const bool bad = a.fixed->bad[t] != 0;
        a.fixed->bad[t] = 0;
        long long q = 0;
        if (a.cphys <= 128) {  // one round trip: two threads per channel, eight shards each; integer sums do not depend on the order
            const int ch = t & 127, s0 = (t >> 7) * 8;
            long long part[8];
#pragma unroll
            for (int sh = 0; sh < 8; ++sh) part[sh] = a.fixed->fix[s0 + sh][ch];
#pragma unroll
            for (int sh = 0; sh < 8; ++sh) {
                q += part[sh];
                a.fixed->fix[s0 + sh][ch] = 0;  // this block is the only reader; the next writers come later in stream order
            }
            if (t >= 128) qs[ch] = q;
            __syncthreads();
            if (t < 128) q += qs[t];
        } else {
#pragma unroll 1
            for (int s0 = 0; s0 < kColShards; s0 += 8) {
                long long part[8];
#pragma unroll
                for (int sh = 0; sh < 8; ++sh) part[sh] = a.fixed->fix[s0 + sh][t];
#pragma unroll
                for (int sh = 0; sh < 8; ++sh) {
                    q += part[sh];
                    a.fixed->fix[s0 + sh][t] = 0;
                }
            }
        }
        const float sum = (float)((double)q * (1.0 / (double)kColScale));
        mean[t] = t < a.cphys ? (bad ? __builtin_nanf("") : sum / (float)a.npix) : 0.0f;
    } else if (a.cphys <= 128) {  // two threads per channel (rows split in halves) keep 256 loads in flight; fixed order
        const int ch = t & 127, half = t >> 7;
        float s = 0.0f;
        if (ch < a.cphys) {
            const int r0 = half ? (a.nparts + 1) / 2 : 0, r1 = half ? a.nparts : (a.nparts + 1) / 2;
#pragma unroll 8
            for (int b = r0; b < r1; ++b) s += a.partial[(size_t)b * a.pstride + ch];
        }
        gv[t] = s;
        __syncthreads();
        mean[t] = t < a.cphys ? (gv[t] + gv[128 + t]) / (float)a.npix : 0.0f;
    } else {
        float s = 0.0f;
        if (t < a.cphys) {
#pragma unroll 8
            for (int b = 0; b < a.nparts; ++b) s += a.partial[(size_t)b * a.pstride + t];
        }
        mean[t] = s / (float)a.npix;
    }
    FOLD_STAMP(1);
    // s: g[t] = bg[t] + sum_c WgT[c][t] * mean[c], then bias'[t] = bf[t] + sum_j WfgT[j][t] * g[j]; each step starts with a barrier
    float s = bg;
    const int total = gs.chunks[0] + gs.chunks[1];
    for (int g = 0; g < total; g += 2) {
        gave_step(a, gs, g, r0, stage, mean, gv, s, bf);
        gave_step(a, gs, g + 1, r1, stage, mean, gv, s, bf);
    }
    if (t < a.bias_len) a.bias_out[t] = t < a.c_out ? s : 0.0f;
    FOLD_STAMP(3);
}

__global__ __launch_bounds__(256) void gave_bias_kernel(const GaveArgs a)
{
    __shared__ f32x4 lds[kGaveLds];
    gave_bias_block(a, reinterpret_cast<float *>(lds));
}

struct PrepArgs {
    const float *values;   // [npix, rows_stride] fusion_values
    const float *weights;  // [npix, rows_stride] fusion_weights
    const float *depth;
    const uint8_t *sem;
    f32x4 *x0;
    f32x4 *x1;
    int rows_stride, in_layout, npix, P, cs4, n_classes, v2_sem;
    int *ovf;  // split-fp16 range guard flag (NULL for fp32 arithmetic)
    int split; // the slots are kept as split planes (dense_chain_kernel)
};

// modules/pipeline.py:74-102 _prepare_fusion_input: channels [values(P) | weights(P) | depth | (sem)]
// packed into the first dense-growth slot of each head; semantic_frame = (1 + id) / n_classes
__global__ __launch_bounds__(256) void prepare_input_kernel(const PrepArgs a)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.npix) return;
    // rows: element (p, c) at [p*stride + c]; sample planes: [c*stride + p]
    const size_t pix = a.in_layout ? (size_t)p : (size_t)p * a.rows_stride;
    const size_t chn = a.in_layout ? (size_t)a.rows_stride : 1;
    const float *v = a.values + pix;
    const float *wt = a.weights + pix;
    const float d = a.depth[p];
    const float sf = a.sem ? (1.0f + (float)a.sem[p]) / (float)a.n_classes : 0.0f;
    bool bad = false;
    for (int cg = 0; cg < a.cs4; ++cg) {
        f32x4 r0, r1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * cg + j;
            float base = 0.0f;
            if (c < a.P) base = v[c * chn];
            else if (c < 2 * a.P) base = wt[(c - a.P) * chn];
            r0[j] = base;
            r1[j] = base;
            if (c == 2 * a.P) { r0[j] = d; r1[j] = sf; }
            if (c == 2 * a.P + 1 && a.v2_sem) r0[j] = sf;
        }
        a.x0[(size_t)cg * a.npix + p] = a.split ? split_pack4(r0) : r0;
        if (a.x1) a.x1[(size_t)cg * a.npix + p] = a.split ? split_pack4(r1) : r1;
        bad = bad || beyond_f16(r0) || beyond_f16(r1);
    }
    if (bad && a.ovf) guard_raise(a.ovf, 1);
}

// rows <-> planes (ojf_conv2d test entry point only)
__global__ __launch_bounds__(256) void rows_to_planes_kernel(const float *rows, int stride, int off, int c, f32x4 *planes,
                                                              int c4, int npix)
{
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= npix * c4) return;
    const int cg = item / npix, p = item - cg * npix;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (4 * cg + j < c) ? rows[(size_t)p * stride + off + 4 * cg + j] : 0.0f;
    planes[(size_t)cg * npix + p] = v;
}

__global__ __launch_bounds__(256) void planes_to_rows_kernel(const f32x4 *planes, int c4, int npix, float *rows, int stride,
                                                              int off)
{
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= npix * c4) return;
    const int cg = item / npix, p = item - cg * npix;
    const f32x4 v = planes[(size_t)cg * npix + p];
#pragma unroll
    for (int j = 0; j < 4; ++j) rows[(size_t)p * stride + off + 4 * cg + j] = v[j];
}

}  // namespace ojf
#include "ojf_net_pair.h"
#include "ojf_net_chain.h"
namespace ojf {

// ------------------------------------------------------------------------------------------------
// host side: packing and the layer schedule
// ------------------------------------------------------------------------------------------------
struct PackedConv {
    float *wp = nullptr;    // device; layout depends on arith
    float *bias = nullptr;  // device, n_ot*16 floats
    float *rinv = nullptr;  // device, n_ot*16 floats (split-fp16 only)
    float *wp_rows = nullptr;  // device; split-fp16 3x3 layers of two output tiles with 3 c4 <= 16: the tap-row stream (rows_form_packed)
    int c_in_phys = 0, c_out_phys = 0, taps = 1, dil = 1, n_ot = 0;
    int arith = OJF_ARITH_F32, nsteps = 0;  // supersteps: 4 (fp32) or 8 (split-fp16) K entries each
};

static int g_default_arith = OJF_ARITH_F16X3;

// Launch log of a forward pass: every launch site calls mark_launch(name, stream) right after its launch.  It counts the
// launches (ojf_net_launch_count) and, in profile mode (ojf_net_profile), records a fence-free timing event behind the
// launch, so that the time between consecutive marks of one stream is that kernel's duration as the stream sees it.
// The names are one table: the launch sites pass an index, the forward plan (plan_launches / ojf_net_plan) lists the same indices.
enum Launch {
    L_DENSE_CHAIN, L_DENSE_PAIR, L_CONV_F16X3, L_CONV_F16X3_GROUPED, L_CONV_MFMA, L_COLSUM, L_GAVE_BIAS, L_ENTRY1X1, L_POOL_PYRAMID,
    L_TAIL, L_TAIL_ENTRY, L_TAIL_HALF_ENTRY, L_TAIL_HEAD, L_COUNT
};
static const char *const kLaunchNames[L_COUNT] = {
    "dense_chain_kernel", "dense_pair_kernel", "conv_f16x3_kernel", "conv_f16x3_kernel (grouped)", "conv_mfma_kernel", "colsum_kernel",
    "gave_bias_kernel", "entry1x1_kernel", "pool_pyramid_kernel", "vortex_tail_kernel",
    "vortex_tail_kernel (+ next entry GEMM)", "vortex_tail_kernel (+ half of the next entry GEMM)", "vortex_tail_kernel (+ prediction head)",
};
// a generic convolution launch of n (<= 4) problems (launch_conv_args)
static inline Launch conv_launch(int arith, int n) { return arith != OJF_ARITH_F16X3 ? L_CONV_MFMA : n > 1 ? L_CONV_F16X3_GROUPED : L_CONV_F16X3; }

struct LaunchMark { const char *name; hipStream_t st; hipEvent_t ev; };
static thread_local int g_launches = 0;
static thread_local bool g_profile = false;
static thread_local std::vector<LaunchMark> g_marks;

static inline void mark_launch(Launch what, hipStream_t st)
{
    ++g_launches;
    if (!g_profile) return;
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    g_marks.push_back(LaunchMark{kLaunchNames[what], st, e});
}

// OJF_NET_TRACE=1 (read once per process, like OJF_SEG_TRACE): one stderr line per launch, "ojf_net <launch name> | <field> <value> ...",
// with the numbers the launch site decided: how it cuts the frame into pixel blocks, bands and tiles.  tests/net_edge_cases.py restates
// those decisions and tests/test_net_edges_gpu.py compares the two.  Unset, nothing changes: the lines are the only effect.
static bool net_trace_on()
{
    static const bool on = getenv("OJF_NET_TRACE") ? atoi(getenv("OJF_NET_TRACE")) != 0 : false;
    return on;
}

// (ojf_net_conv.h)
unsigned event_flags() { return hipEventDisableTiming | hipEventDisableSystemFence; }

// Split-fp16 weights are equilibrated per output channel: row oc is multiplied by the power of two that brings its
// largest magnitude to [2^13, 2^14) before it is split, and the accumulator is multiplied by the inverse in the
// epilogue (both exact).  BN folding scales whole rows by 1/sqrt(var) - without this, rows of ~1e-5 (large input
// channels such as the fp16 weight counts) would sit in the fp16 subnormals and lose their mantissa.
static inline float row_scale(float row_max)
{
    if (!(row_max > 0.0f) || !std::isfinite(row_max)) return 1.0f;
    int e = 0;
    (void)std::frexp(row_max, &e);  // row_max = m * 2^e, m in [0.5, 1)
    int k = 14 - e;
    k = k > 100 ? 100 : (k < -100 ? -100 : k);
    return std::ldexp(1.0f, k);
}

// fp16 halves of a weight, both rounded to nearest (host side of split_f16)
static inline void split_weight(float v, _Float16 &hi, _Float16 &lo)
{
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

struct ConvBuilder {
    int c_in_phys, c_out_phys, taps, dil;
    std::vector<float> W;  // [c_out_phys][taps][c_in_phys]
    std::vector<float> B;
    ConvBuilder(int cin_phys, int cout_phys, int ksize, int dilation)
        : c_in_phys(cin_phys), c_out_phys(cout_phys), taps(ksize * ksize), dil(dilation),
          W((size_t)cout_phys * ksize * ksize * cin_phys, 0.0f), B(cout_phys, 0.0f) {}
    // copy input columns [ci0, ci1) of `L` (all of its output rows) to output rows oc_off..,
    // input column ci -> physical channel in_map[ci - ci0]
    void add(const ojf_conv_layer &L, int ci0, int ci1, const std::vector<int> &in_map, int oc_off, bool with_bias)
    {
        const int kk = L.ksize * L.ksize;
        for (int o = 0; o < L.c_out; ++o) {
            for (int ci = ci0; ci < ci1; ++ci)
                for (int t = 0; t < kk; ++t)
                    W[((size_t)(oc_off + o) * taps + t) * c_in_phys + in_map[ci - ci0]] =
                        L.weight_host[((size_t)o * L.c_in + ci) * kk + t];
            if (with_bias) B[oc_off + o] = L.bias_host[o];
        }
    }
};

static int upload(const std::vector<float> &h, float **d)
{
    OJF_HIP(hipMalloc(reinterpret_cast<void **>(d), h.size() * sizeof(float)));
    OJF_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// layers that get a second weight stream for the row-pair form of the grouped launches (launch_conv_args decides per launch)
static inline bool rows_form_packed(int arith, int taps, int c4, int n_ot)
{
    return arith == OJF_ARITH_F16X3 && taps == 9 && 3 * c4 <= 16 && n_ot == 2;
}

static int finish(const ConvBuilder &b, PackedConv &pc, int arith = OJF_ARITH_F32)
{
    if (b.c_in_phys % 4) return fail("conv packing: c_in_phys must be a multiple of 4");
    pc.c_in_phys = b.c_in_phys;
    pc.c_out_phys = b.c_out_phys;
    pc.taps = b.taps;
    pc.dil = b.dil;
    pc.arith = arith;
    pc.n_ot = round_up(round_up(b.c_out_phys, 16) / 16, kNT);
    const int c4 = b.c_in_phys / 4, groups = b.taps * c4;
    const int per = arith == OJF_ARITH_F16X3 ? 8 : 4;  // K entries per superstep
    const int nsteps = (groups + per - 1) / per;
    if (nsteps > kMaxSteps) return fail("conv packing: K too large for the tap table");
    pc.nsteps = nsteps;
    std::vector<float> wp, bias((size_t)pc.n_ot * 16, 0.0f), rs_rows;
    if (arith == OJF_ARITH_F16X3) {
        std::vector<float> rs((size_t)pc.n_ot * 16, 1.0f), rinv((size_t)pc.n_ot * 16, 1.0f);
        for (int oc = 0; oc < b.c_out_phys; ++oc) {
            float mx = 0.0f;
            const float *row = b.W.data() + (size_t)oc * b.taps * b.c_in_phys;
            for (int i = 0; i < b.taps * b.c_in_phys; ++i) mx = std::fmax(mx, std::fabs(row[i]));
            rs[oc] = row_scale(mx);
            rinv[oc] = 1.0f / rs[oc];
        }
        if (upload(rinv, &pc.rinv)) return -2;
        rs_rows = rs;
        // [S][ot][hi|lo][lane] x 8 halfs; dead (all-zero) supersteps behind for the chunk copies
        const int nsp = nsteps + kPad16;
        wp.assign((size_t)nsp * pc.n_ot * 128 * 4, 0.0f);
        _Float16 *hp = reinterpret_cast<_Float16 *>(wp.data());
        for (int S = 0; S < nsteps; ++S)
            for (int ot = 0; ot < pc.n_ot; ++ot)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int oc = ot * 16 + (lane & 15), G = 8 * S + 2 * (lane >> 4) + (j >> 2);
                        if (oc >= b.c_out_phys || G >= groups) continue;
                        const int t = G / c4, cg = G % c4;
                        const float v = rs[oc] * b.W[((size_t)oc * b.taps + t) * b.c_in_phys + 4 * cg + (j & 3)];
                        const size_t base = ((size_t)S * pc.n_ot + ot) * 2 * 64 * 8;
                        split_weight(v, hp[base + (size_t)lane * 8 + j], hp[base + 64 * 8 + (size_t)lane * 8 + j]);
                    }
    } else {
        const int nsp = nsteps + kPadSteps;  // dead (all-zero) supersteps for the prefetch tail
        wp.assign((size_t)pc.n_ot * nsp * 256, 0.0f);
        for (int ot = 0; ot < pc.n_ot; ++ot)
            for (int S = 0; S < nsteps; ++S)
                for (int lane = 0; lane < 64; ++lane) {
                    const int oc = ot * 16 + (lane & 15), G = 4 * S + (lane >> 4);
                    if (oc >= b.c_out_phys || G >= groups) continue;
                    const int t = G / c4, cg = G % c4;
                    const float *row = b.W.data() + ((size_t)oc * b.taps + t) * b.c_in_phys + 4 * cg;
                    float *dst = wp.data() + (((size_t)ot * nsp + S) * 64 + lane) * 4;
                    for (int j = 0; j < 4; ++j) dst[j] = row[j];
                }
    }
    for (int o = 0; o < b.c_out_phys; ++o) bias[o] = b.B[o];
    if (rows_form_packed(arith, b.taps, c4, pc.n_ot)) {
        // the same hi / lo halves of the same scaled weights in the K order of conv_f16x3_rows_kernel: superstep 2 ky + s,
        // slot 8 s + 2 (lane >> 4) + (j >> 2) = kx * c4 + cg; slots from 3 c4 on stay zero
        std::vector<float> wr((size_t)6 * pc.n_ot * 128 * 4, 0.0f);
        _Float16 *hp = reinterpret_cast<_Float16 *>(wr.data());
        for (int S = 0; S < 6; ++S)
            for (int ot = 0; ot < pc.n_ot; ++ot)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int oc = ot * 16 + (lane & 15), slot = 8 * (S & 1) + 2 * (lane >> 4) + (j >> 2);
                        if (oc >= b.c_out_phys || slot >= 3 * c4) continue;
                        const int t = 3 * (S >> 1) + slot / c4, cg = slot % c4;
                        const float v = rs_rows[oc] * b.W[((size_t)oc * b.taps + t) * b.c_in_phys + 4 * cg + (j & 3)];
                        const size_t base = ((size_t)S * pc.n_ot + ot) * 2 * 64 * 8;
                        split_weight(v, hp[base + (size_t)lane * 8 + j], hp[base + 64 * 8 + (size_t)lane * 8 + j]);
                    }
        if (upload(wr, &pc.wp_rows)) return -2;
    }
    if (upload(wp, &pc.wp)) return -2;
    if (upload(bias, &pc.bias)) return -2;
    return 0;
}

static void release(PackedConv &pc)
{
    if (pc.wp) (void)hipFree(pc.wp);
    if (pc.bias) (void)hipFree(pc.bias);
    if (pc.rinv) (void)hipFree(pc.rinv);
    if (pc.wp_rows) (void)hipFree(pc.wp_rows);
    pc.wp = pc.bias = pc.rinv = pc.wp_rows = nullptr;
}

// ---- fused 3x3 -> 3x3 pair (dense_pair_kernel, ojf_net_pair.h) ----------------------------------------------------
#ifdef OJF_PAIR_TIMING
static long long *g_pair_dbg = nullptr;
#endif
struct PackedPair {
    float *wa = nullptr, *wb = nullptr, *vec = nullptr;  // vec: bias_a | rinv_a | bias_b | rinv_b (32 floats each)
    int c4_in = 0, n_chunks = 0, np_last = 0, np_b = 0, og_store = 0;
    int cfg = 0;  // PairCfg of the launches
};

// Launch shapes of dense_pair_kernel (PairGeom): picked per frame size
enum PairCfg { PAIR_20x16_W16 = 0, PAIR_12x8_W16 = 1 };
constexpr int kPairChunkPairs = 4;  // channel pairs per chunk of the first convolution's packed weights (PairGeom::CP)
static int pair_cfg_for(int h, int w)
{
    // one block per tile, 16 waves: the large tile when it still gives every CU a block (320x240: 240 blocks)
    // (round 4 measured other shapes - two 8-wave blocks per CU, packed rows - against this one: DESIGN.md §5.0, no gain)
    return ((w + 19) / 20) * ((h + 15) / 16) >= 200 ? PAIR_20x16_W16 : PAIR_12x8_W16;
}

static void release(PackedPair &pp)
{
    float *ptrs[] = {pp.wa, pp.wb, pp.vec};
    for (float *p : ptrs)
        if (p) (void)hipFree(p);
    pp.wa = pp.wb = pp.vec = nullptr;
}

// K blocks of `np_chunk`-pair chunks: unit u = 4S + g -> (tap = u / np, pair = u % np), K slot j = channel 8*pair + j
static void pack_pair_conv(const ConvBuilder &b, const std::vector<float> &rs, std::vector<float> &dst, int cp)
{
    const int npairs = (b.c_in_phys + 7) / 8, n_chunks = (npairs + cp - 1) / cp;
    for (int c = 0; c < n_chunks; ++c) {
        const int np = c == n_chunks - 1 ? npairs - cp * c : cp, nkb = (9 * np + 3) / 4;
        const size_t base = dst.size();
        dst.resize(base + (size_t)nkb * 256 * 4, 0.0f);
        _Float16 *hp = reinterpret_cast<_Float16 *>(dst.data() + base);
        for (int S = 0; S < nkb; ++S)
            for (int nt = 0; nt < 2; ++nt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int oc = nt * 16 + (lane & 15), u = 4 * S + (lane >> 4);
                        if (oc >= b.c_out_phys || u >= 9 * np) continue;
                        const int tap = u / np, ch = 8 * (cp * c + u % np) + j;
                        if (ch >= b.c_in_phys) continue;
                        const float v = rs[oc] * b.W[((size_t)oc * b.taps + tap) * b.c_in_phys + ch];
                        const size_t ub = ((size_t)S * 2 + nt) * 2 * 64 * 8;
                        split_weight(v, hp[ub + (size_t)lane * 8 + j], hp[ub + 64 * 8 + (size_t)lane * 8 + j]);
                    }
    }
}

static int finish_pair(const ConvBuilder &ba, const ConvBuilder &bb, PackedPair &pp, int cfg = PAIR_20x16_W16)
{
    constexpr int cp = kPairChunkPairs;
    pp.cfg = cfg;
    if (ba.taps != 9 || bb.taps != 9 || ba.dil != 1 || bb.dil != 1 || ba.c_out_phys > 24 || bb.c_in_phys != ba.c_out_phys ||
        bb.c_out_phys > 32 || ba.c_in_phys % 4)
        return fail("pair packing: unsupported layer shapes");
    std::vector<float> vec(128, 0.0f), wa, wb;
    auto scales = [&](const ConvBuilder &b, int off) {
        std::vector<float> rs(32, 1.0f);
        for (int oc = 0; oc < b.c_out_phys; ++oc) {
            float mx = 0.0f;
            const float *row = b.W.data() + (size_t)oc * b.taps * b.c_in_phys;
            for (int i = 0; i < b.taps * b.c_in_phys; ++i) mx = std::fmax(mx, std::fabs(row[i]));
            rs[oc] = row_scale(mx);
            vec[off + oc] = b.B[oc];
        }
        for (int oc = 0; oc < 32; ++oc) vec[off + 32 + oc] = 1.0f / rs[oc];
        return rs;
    };
    const std::vector<float> ra = scales(ba, 0), rb = scales(bb, 64);
    pack_pair_conv(ba, ra, wa, cp);
    pack_pair_conv(bb, rb, wb, cp);  // (3 pairs: one chunk)
    pp.np_b = (bb.c_in_phys + 7) / 8;
    const int npairs = (ba.c_in_phys + 7) / 8;
    pp.c4_in = ba.c_in_phys / 4;
    pp.n_chunks = (npairs + cp - 1) / cp;
    pp.np_last = npairs - cp * (pp.n_chunks - 1);
    pp.og_store = round_up(bb.c_out_phys, 4) / 4;
    if (upload(wa, &pp.wa) || upload(wb, &pp.wb) || upload(vec, &pp.vec)) return -2;
    return 0;
}

template <int TW, int TH>
static int launch_pair_t(PairArgs &a, hipStream_t st)
{
    using G = PairGeom<TW, TH>;
    static_assert(G::CP == kPairChunkPairs, "the weights are packed in chunks of PairGeom::CP channel pairs");
    static bool configured = false;
    if (!configured) {
        OJF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&dense_pair_kernel<TW, TH>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES));
        configured = true;
    }
    a.tiles_x = (a.w + TW - 1) / TW;
    const int tiles = a.tiles_x * ((a.h + TH - 1) / TH);
    if (net_trace_on())
        fprintf(stderr, "ojf_net %s | tw %d th %d tiles_x %d tiles %d grid_x %d banded %d\n", kLaunchNames[L_DENSE_PAIR], TW, TH, a.tiles_x, tiles,
                tiles, (tiles & 7) == 0 ? 1 : 0);
    hipLaunchKernelGGL((dense_pair_kernel<TW, TH>), dim3(tiles), dim3(G::THREADS), G::LDS_BYTES, st, a);
    mark_launch(L_DENSE_PAIR, st);
    return check_hip(hipGetLastError(), "dense_pair_kernel launch");
}

// in / out: plane buffers (may be the same allocation: the output groups are not part of the input window)
static int launch_pair(const PackedPair &pp, const float *in, int in_g0, float *out, int out_g0, int h, int w, hipStream_t st)
{
    PairArgs a;
    a.in = planes(in); a.out = planes(out);
    a.wa = planes(pp.wa); a.wb = planes(pp.wb);
    a.bias_a = pp.vec; a.rinv_a = pp.vec + 32; a.bias_b = pp.vec + 64; a.rinv_b = pp.vec + 96;
    a.in_g0 = in_g0; a.c4_in = pp.c4_in; a.out_g0 = out_g0; a.og_store = pp.og_store;
    a.h = h; a.w = w; a.npix = h * w; a.tiles_x = 0;
    a.n_chunks = pp.n_chunks; a.np_last = pp.np_last; a.np_b = pp.np_b;
    a.ovf = overflow_flag();
#ifdef OJF_PAIR_TIMING
    a.dbg = g_pair_dbg;
#endif
    switch (pp.cfg) {
    case PAIR_20x16_W16: return launch_pair_t<20, 16>(a, st);
    case PAIR_12x8_W16: return launch_pair_t<12, 8>(a, st);
    }
    return fail("dense pair: unknown launch shape");
}

// ---- all dense Blocks of a head in one persistent launch (dense_chain_kernel, ojf_net_chain.h) ---------------------
#ifdef OJF_CHAIN_TIMING
static long long *g_chain_dbg = nullptr;
#endif
struct PackedChain {
    float *w = nullptr, *vec = nullptr;
    int *sync = nullptr;  // ChainDenseArgs::sync
    int layers = 0;
};
constexpr int kChainSyncInts = kChainFlags0 + 8192;

static void release(PackedChain &pc)
{
    if (pc.w) (void)hipFree(pc.w);
    if (pc.vec) (void)hipFree(pc.vec);
    if (pc.sync) (void)hipFree(pc.sync);
    pc.w = pc.vec = nullptr; pc.sync = nullptr; pc.layers = 0;
}

// one step of dense_chain_kernel: input channels [ch0, ch0 + 20) of `b`, [K block][packed row tile][lane] x 8 halfs;
// packed row tiles (ojf_net_chain.h): 0 = hi halves of channels 0..15, 1 = their lo halves, 2 = hi | lo halves of channels
// 16..19 in rows 0..3 | 4..7; lane (row r16, lane group g), half j: position (R = 2 S + j / 4, g) -> (tap, channel group),
// input channel 4 q + j % 4
static void pack_chain_step(const ConvBuilder &b, const std::vector<float> &rs, int ch0, std::vector<float> &dst)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)kChainStepF4 * 4, 0.0f);
    _Float16 *hp = reinterpret_cast<_Float16 *>(dst.data() + base);
    for (int S = 0; S < kChainKB; ++S)
        for (int t = 0; t < 3; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int r16 = lane & 15, g = lane >> 4, R = 2 * S + (j >> 2);
                    const int oc = t < 2 ? r16 : (r16 < 8 ? 16 + (r16 & 3) : -1);
                    const bool want_lo = t == 1 || (t == 2 && r16 >= 4);
                    const int tap = chain_hu_tap(R, g), ch = ch0 + 4 * chain_hu_q(R, g) + (j & 3);
                    if (oc < 0 || oc >= b.c_out_phys || tap < 0 || ch >= b.c_in_phys) continue;
                    const float v = rs[oc] * b.W[((size_t)oc * b.taps + tap) * b.c_in_phys + ch];
                    _Float16 hi, lo;
                    split_weight(v, hi, lo);
                    hp[(((size_t)S * 3 + t) * 64 + lane) * 8 + j] = want_lo ? lo : hi;
                }
}

// ba[l] / bb[l]: the two convolutions of Block l (ba[l].c_in_phys = 20 (l + 1), everything else 20 channels)
static int finish_chain(const std::vector<ConvBuilder> &ba, const std::vector<ConvBuilder> &bb, PackedChain &pc)
{
    const int L = (int)ba.size();
    if (L < 1 || L > kChainMaxLayers || (int)bb.size() != L) return fail("chain packing: unsupported Block count");
    std::vector<float> vec((size_t)L * 128, 0.0f), w;
    for (int l = 0; l < L; ++l) {
        const ConvBuilder &a = ba[l], &b = bb[l];
        if (a.taps != 9 || b.taps != 9 || a.dil != 1 || b.dil != 1 || a.c_out_phys != 4 * kChainNG || b.c_in_phys != 4 * kChainNG ||
            b.c_out_phys != 4 * kChainNG || a.c_in_phys != 4 * kChainNG * (l + 1))
            return fail("chain packing: unsupported layer shapes");
        auto scales = [&](const ConvBuilder &cb, int off) {
            std::vector<float> rs(32, 1.0f);
            for (int oc = 0; oc < cb.c_out_phys; ++oc) {
                float mx = 0.0f;
                const float *row = cb.W.data() + (size_t)oc * cb.taps * cb.c_in_phys;
                for (int i = 0; i < cb.taps * cb.c_in_phys; ++i) mx = std::fmax(mx, std::fabs(row[i]));
                rs[oc] = row_scale(mx);
                vec[(size_t)l * 128 + off + oc] = cb.B[oc];
            }
            for (int oc = 0; oc < 32; ++oc) vec[(size_t)l * 128 + off + 32 + oc] = 1.0f / rs[oc];
            return rs;
        };
        const std::vector<float> ra = scales(a, 0), rb = scales(b, 64);
        for (int c = 0; c <= l; ++c) pack_chain_step(a, ra, 4 * kChainNG * c, w);
        pack_chain_step(b, rb, 0, w);
    }
    pc.layers = L;
    if (upload(w, &pc.w) || upload(vec, &pc.vec)) return -2;
    OJF_HIP(hipMalloc(reinterpret_cast<void **>(&pc.sync), kChainSyncInts * sizeof(int)));
    OJF_HIP(hipMemset(pc.sync, 0, kChainSyncInts * sizeof(int)));
    OJF_HIP(hipStreamSynchronize(nullptr));  // (see alloc_planes)
    const int epoch0 = kChainEpoch;
    OJF_HIP(hipMemcpy(pc.sync, &epoch0, sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

static int device_cu_count()
{
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    }
    return cus;
}

template <int TW, int TH, int WAVES>
static int launch_chain_t(ChainDenseArgs &a, hipStream_t st)
{
    using G = ChainGeom<TW, TH, WAVES>;
    static bool configured = false;
    if (!configured) {
        OJF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&dense_chain_kernel<TW, TH, WAVES>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES));
        configured = true;
    }
    a.tiles_x = (a.w_img + TW - 1) / TW;
    a.tiles_y = (a.h + TH - 1) / TH;
    const int tiles = a.tiles_x * a.tiles_y, cus = device_cu_count();
    if (tiles > kChainSyncInts - kChainFlags0) return fail("dense chain: too many tiles for the flag array");
    // one block per CU (160 KB of LDS); the blocks draw (Block, tile) items until none is left
    const int grid = cus > 0 && cus < tiles ? cus : tiles;
    if (net_trace_on())
        fprintf(stderr, "ojf_net %s | tw %d th %d tiles_x %d tiles_y %d tiles %d grid_x %d\n", kLaunchNames[L_DENSE_CHAIN], TW, TH, a.tiles_x,
                a.tiles_y, tiles, grid);
    hipLaunchKernelGGL((dense_chain_kernel<TW, TH, WAVES>), dim3(grid), dim3(G::THREADS), G::LDS_BYTES, st, a);
    mark_launch(L_DENSE_CHAIN, st);
    return check_hip(hipGetLastError(), "dense_chain_kernel launch");
}

// x: the dense-growth buffer as split planes (slot 0 filled; slots 1..layers are written)
static int launch_chain(const PackedChain &pc, float *x, int h, int w, hipStream_t st)
{
    ChainDenseArgs a;
    a.x = planes(x); a.xo = planes(x);
    a.w = planes(pc.w); a.vec = pc.vec;
    a.sync = pc.sync; a.layers = pc.layers;
    a.h = h; a.w_img = w; a.npix = h * w; a.tiles_x = a.tiles_y = 0;
    a.ovf = overflow_flag();
#ifdef OJF_CHAIN_TIMING
    a.dbg = g_chain_dbg;
#endif
    if (((w + 19) / 20) * ((h + 15) / 16) >= 200)  // (the large tile when it still gives every CU an item per Block; 16 waves: 12 and 8 measured slower)
        return launch_chain_t<20, 16, 16>(a, st);
    return launch_chain_t<12, 8, 8>(a, st);
}

// (declared in ojf_net_conv.h: the training path launches its convolutions here too)
int launch_conv_args(const ConvArgs *args, int n, int nt, hipStream_t st, int arith)
{
    ConvGroup grp;
    for (int i = 0; i < n; ++i) grp.g[i] = args[i];
    for (int i = n; i < 4; ++i) grp.g[i] = args[0];
    grp.nblocks = 0;
    // one wave computes ALL output-channel tiles of its pixel strip (activations are fetched once);
    // MT (16-pixel tiles per wave) trades operand reuse against the number of waves in flight.
    // fp32: MT = 1 everywhere: 4800 waves over 1024 SIMDs quantise to 5 rounds where MT = 2 (2400 waves) needs 3
    // rounds of twice the length (78 % vs 94 % balance); measured 14.9 vs 17.3 us on the 19->19 3x3 layers.
    // split-fp16: two pixel tiles per wave share the LDS weight reads and the per-wave prologue; measured in one run
    // (net stage): MT = 2 everywhere 0.501 ms, MT = 2 only for grouped / wide launches 0.508 ms, MT = 1 0.514 ms.
    // The wide launches of the training executor (NT >= 6: 96 / 128 output channels) need 204-212 + 64 registers at MT = 2 -
    // one wave per SIMD, nothing to run while a block waits for its weight chunk; MT = 1 (140 + 32) keeps two: training
    // frame step 216 -> 220 and 204 -> 217 frames/s on two boxes (NT <= 4: no difference).
    const int mt = arith == OJF_ARITH_F16X3 ? (nt >= 6 ? 1 : 2) : 1;
    const int strips = (args[0].npix + mt * 16 - 1) / (mt * 16);
    const dim3 grid((strips + 3) / 4, n), block(256);
#define OJF_LAUNCH32(NT_) hipLaunchKernelGGL((conv_mfma_kernel<1, NT_>), grid, block, 0, st, grp)
    int max_steps = 0;
    for (int i = 0; i < n; ++i) max_steps = args[i].nsteps > max_steps ? args[i].nsteps : max_steps;
    const size_t tab_bytes = (size_t)(max_steps + kPad16) * 8 * sizeof(int2);  // (no measurable effect vs the full 8.6 KB)
    // split-fp16 launches hand every XCD one band of the image (xcd_band_block)
    dim3 grid16 = grid;
    if (arith == OJF_ARITH_F16X3 && grid.x >= 64) {
        grp.nblocks = (int)grid.x;
        grid16.x = round_up((int)grid.x, 8);
    }
    if (grp.nblocks)
        for (int i = 0; i < n; ++i) {
            ConvArgs &g = grp.g[i];
            if (g.taps == 9 && g.dil > 1 && g.dil < g.h && g.w % (mt * 16) == 0) {
                g.row_perm = g.dil; g.perm_q = g.h / g.dil; g.perm_rem = g.h % g.dil;
            }
        }
    // persistent blocks for single-chunk layers (ConvGroup::band): `bpc` blocks per CU over all members of the group
    constexpr int persist_bpc = 3;  // measured 2 / 3 / 4 / 6 and one pixel block per launch block: 3 is best (profiles/r06_fusion_net_experiments.txt)
    if (grp.nblocks && arith == OJF_ARITH_F16X3) {
        bool single = true;
        for (int i = 0; i < n; ++i) single = single && args[i].nsteps <= conv16_chunk(nt);
        const int cus = device_cu_count();
        const int n8 = round_up(grp.nblocks, 8);
        int G = cus > 0 ? (cus * persist_bpc / n) / 8 * 8 : 0;
        if (single && G >= 8 && G < n8) {
            grp.band = n8 / 8;
            grid16.x = (unsigned)G;
        }
    }
    bool lean = arith == OJF_ARITH_F16X3;
    for (int i = 0; i < n && lean; ++i) lean = conv_lean_ok(args[i]);
    int n_ins = 0, n_outs = 0;
    for (int i = 0; i < n; ++i) { n_ins += args[i].in_split ? 1 : 0; n_outs += args[i].out_split ? 1 : 0; }
    if (net_trace_on()) {
        char perm[128];
        int at = 0;
        for (int i = 0; i < n; ++i)
            at += snprintf(perm + at, sizeof(perm) - (size_t)at, "%s%d:%d:%d", i ? "," : "", grp.g[i].row_perm, grp.g[i].perm_q, grp.g[i].perm_rem);
        fprintf(stderr, "ojf_net %s | n %d mt %d nt %d grid_x %u nblocks %d grid16_x %u band %d lean %d perm %s\n", kLaunchNames[conv_launch(arith, n)],
                n, mt, nt, grid.x, grp.nblocks, grid16.x, grp.band, lean ? 1 : 0, perm);
    }
    // Row-pair form (conv_f16x3_rows_kernel): decided for the launch as a whole; the grid, the bands and the trace line above are
    // those of the old form - with w % 64 == 0 and h even, (h / 2)(w / 64) pairs-by-column-groups == nblocks.
    bool rows = arith == OJF_ARITH_F16X3 && n_ins == n && mt == 2 && nt == 2 && lean && grp.nblocks > 0 && args[0].w % 64 == 0 && args[0].h % 2 == 0;
    for (int i = 0; i < n && rows; ++i) rows = args[i].wp_rows && args[i].taps == 9 && 3 * args[i].c4 <= 16;
    if ((n_ins || n_outs) && (arith != OJF_ARITH_F16X3 || (n_ins && (n_ins != n || mt != 2 || nt != 2))))
        return fail("conv: split planes are a format of the split-fp16 grouped 3x3 launches only");
#define OJF_LAUNCH16(MT_, NT_)                                                                                      \
    do {                                                                                                             \
        if (lean) hipLaunchKernelGGL((conv_f16x3_kernel<MT_, NT_, true, 0, true>), grid16, block, tab_bytes, st, grp); \
        else hipLaunchKernelGGL((conv_f16x3_kernel<MT_, NT_>), grid16, block, tab_bytes, st, grp);                   \
    } while (0)
    if (arith == OJF_ARITH_F16X3 && mt == 2) {
        switch (nt) {
            case 2:
                if (rows) hipLaunchKernelGGL(conv_f16x3_rows_kernel, grid16, block, 0, st, grp);
                else if (n_ins && lean) hipLaunchKernelGGL((conv_f16x3_kernel<2, 2, true, 0, true, true>), grid16, block, tab_bytes, st, grp);
                else if (n_ins) hipLaunchKernelGGL((conv_f16x3_kernel<2, 2, true, 0, false, true>), grid16, block, tab_bytes, st, grp);
                else OJF_LAUNCH16(2, 2);
                break;
            case 4: OJF_LAUNCH16(2, 4); break;
            case 6: OJF_LAUNCH16(2, 6); break;
            case 8: OJF_LAUNCH16(2, 8); break;
            default: return fail("conv: unsupported number of output tiles");
        }
    } else if (arith == OJF_ARITH_F16X3) {
        switch (nt) {
            case 2: OJF_LAUNCH16(1, 2); break;
            case 4: OJF_LAUNCH16(1, 4); break;
            case 6: OJF_LAUNCH16(1, 6); break;
            case 8: OJF_LAUNCH16(1, 8); break;
            default: return fail("conv: unsupported number of output tiles");
        }
    } else {
        switch (nt) {
            case 2: OJF_LAUNCH32(2); break;
            case 4: OJF_LAUNCH32(4); break;
            case 6: hipLaunchKernelGGL((conv_mfma_lds_kernel<6>), grid, block, 0, st, grp); break;
            case 8: hipLaunchKernelGGL((conv_mfma_lds_kernel<8>), grid, block, 0, st, grp); break;
            default: return fail("conv: unsupported number of output tiles");
        }
    }
#undef OJF_LAUNCH32
#undef OJF_LAUNCH16
    mark_launch(conv_launch(arith, n), st);
    return check_hip(hipGetLastError(), "conv kernel launch");
}

// (ojf_net_conv.h)
unsigned div_magic(int d, uint64_t limit)
{
    if (d <= 1 || limit * (uint64_t)d >= (1ull << 32)) return 0;
    return (unsigned)(((1ull << 32) + (uint64_t)d - 1) / (uint64_t)d);
}

static void fill_conv_args(ConvArgs &a, const PackedConv &pc, const float *in, int in_g0, float *out, int out_g0,
                           const float *bias, int act, int act_n, float scale, int h, int w)
{
    a.ovf = pc.arith == OJF_ARITH_F16X3 ? overflow_flag() : nullptr;
    a.accum = 0; a.dscale = nullptr;
    a.in = planes(in); a.out = planes(out); a.out_rows = nullptr;
    a.wp = planes(pc.wp); a.bias = bias ? bias : pc.bias; a.rinv = pc.rinv;
    a.wp_rows = planes(pc.wp_rows);
    a.in_g0 = in_g0; a.out_g0 = out_g0; a.rows_stride = 0; a.rows_n = 0;
    a.h = h; a.w = w; a.npix = h * w;
    a.taps = pc.taps; a.dil = pc.dil;
    a.c4 = pc.c_in_phys / 4; a.nsteps = pc.nsteps;
    a.w_magic = div_magic(w, (uint64_t)h * w);
    a.c4_magic = div_magic(a.c4, (uint64_t)(pc.nsteps + kPad16) * 8);
    a.og_store = round_up(pc.c_out_phys, 4) / 4;
    a.act = act; a.act_n = act_n; a.scale = scale;
}

// in / out: plane buffers; in_g0 / out_g0: first channel group of the window.
// rows != NULL: the result goes to row-major scalars instead (last layer -> caller's est rows).
static int launch_conv(const PackedConv &pc, const float *in, int in_g0, float *out, int out_g0, const float *bias,
                       int act, int act_n, float scale, int h, int w, hipStream_t st, float *rows = nullptr,
                       int rows_stride = 0, int rows_n = 0)
{
    ConvArgs a;
    fill_conv_args(a, pc, in, in_g0, out, out_g0, bias, act, act_n, scale, h, w);
    a.out_rows = rows; a.rows_stride = rows_stride; a.rows_n = rows_n;
    return launch_conv_args(&a, 1, pc.n_ot, st, pc.arith);
}

static std::vector<int> slot_map(int n_logical, int group, int slot)
{   // logical channel j of a concatenation of `group`-wide tensors stored in `slot`-wide slots
    std::vector<int> m(n_logical);
    for (int j = 0; j < n_logical; ++j) m[j] = (j / group) * slot + (j % group);
    return m;
}

// per-output-row power-of-two scales of a pointwise layer (ones for fp32 arithmetic); n_k input channels
template <class F>
static std::vector<float> chain_row_scales(int arith, int nt_out, int n_k, F weight)
{
    std::vector<float> r((size_t)nt_out * 16, 1.0f);
    if (arith != OJF_ARITH_F16X3) return r;
    for (int oc = 0; oc < nt_out * 16; ++oc) {
        float mx = 0.0f;
        for (int k = 0; k < n_k; ++k) mx = std::fmax(mx, std::fabs(weight(oc, k)));
        r[oc] = row_scale(mx);
    }
    return r;
}

// Fragments of one pointwise layer for chain_layer, appended to dst; weight(oc, k) returns 0 outside the layer,
// rs = row scales (chain_row_scales).
template <class F>
static void pack_chain_layer(std::vector<float> &dst, int arith, int nt_out, int nt_in, const std::vector<float> &rs, F weight)
{
    const size_t base = dst.size();
    dst.resize(base + (size_t)chain_layer_size(arith, nt_in, nt_out) * 4, 0.0f);
    if (arith == OJF_ARITH_F16X3) {
        const int KB = chain_kblocks(arith, nt_in);
        _Float16 *hp = reinterpret_cast<_Float16 *>(dst.data() + base);
        for (int n2 = 0; n2 < nt_out; ++n2)
            for (int S = 0; S < KB; ++S)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int oc = n2 * 16 + (lane & 15), g = lane >> 4;
                        const int k = 32 * S + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
                        const size_t ub = ((size_t)n2 * KB + S) * 2 * 64 * 8;
                        split_weight(rs[oc] * weight(oc, k), hp[ub + (size_t)lane * 8 + j], hp[ub + 64 * 8 + (size_t)lane * 8 + j]);
                    }
    } else {
        for (int n2 = 0; n2 < nt_out; ++n2)
            for (int S = 0; S < nt_in; ++S)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j)
                        dst[base + (((size_t)n2 * nt_in + S) * 64 + lane) * 4 + j] =
                            weight(n2 * 16 + (lane & 15), 16 * S + 4 * (lane >> 4) + j);
    }
}

// bias stream entry of a chain layer: bias[nt_out*16] and, for split-fp16, the inverse row scales behind it
static void append_chain_bias(std::vector<float> &dst, int arith, int nt_out, int c_out, const float *bias_host,
                              const std::vector<float> &rs)
{
    const size_t bb = dst.size();
    dst.resize(bb + (size_t)chain_bias_stride(arith, nt_out), 0.0f);
    for (int o = 0; o < c_out; ++o) dst[bb + o] = bias_host[o];
    if (arith == OJF_ARITH_F16X3)
        for (int o = 0; o < nt_out * 16; ++o) dst[bb + (size_t)nt_out * 16 + o] = 1.0f / rs[o];
}

// ---- the forward plan -------------------------------------------------------------------------------------------------
// Which launches a forward pass consists of depends on the net's shape alone.  plan_forward decides it once, in ojf_net_create
// (and in ojf_net_plan, which needs no device); the packing code asks the same predicates which forms to pack, and
// forward_launches / run_vortex only execute the plan.  A new variant starts here: a predicate for the shapes it serves, a value
// of the step's enum, its case in plan_forward and plan_launches, its packing and its case in the executor.
struct NetShape {
    int version, P, gf, sem, h, w, arith;
    int c, cs, heads, pool_in, os, npix;  // derived (net_shape): channels of a Block and their padded slot, (gf+1)*c and its slot
    int c_in_phys(int k) const { return k < 2 ? (gf + 1) * cs : heads * os; }  // input planes of VortexPooling k (2 = the last one)
};

// nullptr, or why the shape is refused (text after "<entry point>: ")
static const char *net_shape(NetShape &s, int version, int n_points, int growth, int use_semantics, int h, int w, int arith)
{
    if (version != 2 && version != 3) return "version must be 2 or 3";
    if (n_points < 1 || growth < 1 || h <= 0 || w <= 0) return "bad sizes";
    s.version = version; s.P = n_points; s.gf = growth; s.sem = use_semantics ? 1 : 0; s.h = h; s.w = w; s.arith = arith;
    s.c = 2 * n_points + 1 + (version == 2 ? s.sem : 0);
    s.cs = round_up(s.c, 4);
    s.heads = (version == 3 && s.sem) ? 2 : 1;
    s.pool_in = s.c * (growth + 1);
    s.os = round_up(s.pool_in, 4);
    s.npix = h * w;
    if (s.heads * s.os > 256 || (growth + 1) * s.cs > 256) return "topology too wide";
    return nullptr;
}

// The test-only switch OJF_NO_DENSE_CHAIN (set = present in the environment), read once per process (the tests that set it start
// child processes)
static bool no_dense_chain()
{
    static const bool set = getenv("OJF_NO_DENSE_CHAIN") != nullptr;
    return set;
}

// Shape predicates: each form of the packing code exists exactly where its predicate holds.
// input tiles of a VortexPooling's entry GEMM as one chain layer (entry1x1_kernel / the previous tail): 8, 16 (the two-head net's
// last VortexPooling, 228 = 2 x 114 input channels), or 0 = no such form (generic stacked convolution)
static int entry_tiles(int c_in_phys, int cs) { return c_in_phys <= 256 && 4 * cs <= 80 ? (c_in_phys <= 128 ? 8 : 16) : 0; }
// ... split into one 8-tile layer per head, run by the two heads' tails
static bool half_entry_form(int c_in_phys, int cs, int os) { return entry_tiles(c_in_phys, cs) == 16 && c_in_phys == 2 * os; }
// fused tail (vortex_tail_kernel): 2 branch tiles, 8 output tiles
static bool fused_tail_form(int cs, int os) { return (cs + 15) / 16 == 2 && (os + 15) / 16 == 8; }
// chain flow of VortexPooling k: entry and tail both have their chain-layer forms
static bool chain_flow_form(const NetShape &s, int k) { return entry_tiles(s.c_in_phys(k), s.cs) != 0 && fused_tail_form(s.cs, s.os); }
// dense Blocks as dense_pair_kernel launches / as one dense_chain_kernel launch
static bool pair_form(const NetShape &s) { return s.arith == OJF_ARITH_F16X3 && s.cs <= 24; }
static bool chain_form(const NetShape &s) { return pair_form(s) && s.cs == 4 * kChainNG && s.gf <= kChainMaxLayers; }
// growth channels of the prediction head as chain layers inside the last tail (19 / 20), 0 = layer by layer
static int chain_kind_of(const NetShape &s) { return s.P == 9 && s.gf == 5 && (s.c == 19 || s.c == 20) ? s.c : 0; }
// One dense_chain_kernel launch per head instead of gf dense_pair_kernel launches: the dense-growth buffers then hold split
// planes, which only the chain-flow entry kernel reads.
static bool chain_dense_form(const NetShape &s)
{
    if (s.arith != OJF_ARITH_F16X3 || no_dense_chain()) return false;
    //  frames the chain kernel is not the right tool for fall back to one dense_pair_kernel launch per Block:
    //  * more tiles than the flag array holds (frames beyond ~2.6 Mpixel used to fail in ojf_net_forward);
    //  * w % 8 != 0: a 128-byte line of a plane is 8 pixels, so a line then straddles two image rows - pixels of tiles
    //    whose flags a reader never checked - and only the slot of the Block just finished is read with sc1 loads: an
    //    early reader could pull a not-yet-written pixel of an OLDER slot into its XCD's L2 and a later item read it stale.
    const int big = ((s.w + 19) / 20) * ((s.h + 15) / 16);
    const int tiles = big >= 200 ? big : ((s.w + 11) / 12) * ((s.h + 7) / 8);
    if (tiles > kChainSyncInts - kChainFlags0 || (s.w % 8) != 0) return false;
    return chain_form(s) && chain_flow_form(s, 0);  // (every head's VortexPooling has the shape of the first)
}

enum DenseKind { DENSE_CHAIN, DENSE_PAIRS, DENSE_CONVS };
enum EntryKind { ENTRY_KERNEL, ENTRY_BY_PREV_TAIL, ENTRY_GENERIC };
enum BranchKind { BRANCH_GROUPED, BRANCH_GROUPED_SIDE0 };
enum TailKind { TAIL_UNFUSED, TAIL_ALONE, TAIL_ENTRY, TAIL_HALF_ENTRY, TAIL_HEAD };

struct VortexStep {
    int vortex, set;  // net->vortex[vortex] on net->sc[set]; steps 0 / 1 are heads 0 / 1 behind their dense Blocks, 2 is the last one
    // Chain flow (no side stream, no events): entry GEMM + column sums in one chain-layer launch (or inside the previous
    // tail), the global-average fold as one extra block of the pyramid launch, all four branches in the grouped launches.
    // General flow (topologies whose entry or tail has no chain-layer form): generic convolutions, the global-average branch
    // on the side stream.
    bool chain_flow;
    EntryKind entry;  // ENTRY_KERNEL: entry1x1_kernel with entry_ntin input tiles; ENTRY_GENERIC: + the two global-average kernels
    int entry_ntin;
    bool in_split;    // the input holds split planes (dense_chain_kernel's result)
    // split planes between the branch-entry producers (entry GEMM: branch 0; pool pyramid: branches 1-3), the branches' first
    // 3x3 and their second 3x3 (whose result the tail reads as plain fp32 planes)
    bool split;
    BranchKind branches;  // BRANCH_GROUPED_SIDE0: branch 0 needs no pooling, its 3x3 pair follows the global-average kernels on the side stream
    TailKind tail;    // TAIL_UNFUSED: four 1x1 + the final convolution through Scratch::CAT; the others: vortex_tail_kernel and what rides along
    int half;         // TAIL_HALF_ENTRY: which half of the last entry GEMM (channel sums into net->colsum3 at half * os)
    bool z2;          // the pyramid adds the other head's partial entry planes (sc[1].Z) and forms branch 0 (Q0, bias0); channel sums: net->colsum3
};

struct ForwardPlan {
    DenseKind dense;
    int n_steps;         // 2, or 3 = two heads: step 0 (head 1, on its own stream), step 1 (head 0), step 2
    VortexStep step[3];  // in host enqueue order
    bool head_layers;    // the prediction head runs layer by layer afterwards (PA / PB)
    int chain_kind;
};

// nullptr, or the refusal (ojf_net_create fails with it)
static const char *plan_forward(const NetShape &s, ForwardPlan *plan)
{
    const bool h16 = s.arith == OJF_ARITH_F16X3, two = s.heads == 2, fused = fused_tail_form(s.cs, s.os);
    ForwardPlan &p = *plan;
    p.dense = chain_dense_form(s) ? DENSE_CHAIN : pair_form(s) ? DENSE_PAIRS : DENSE_CONVS;
    p.chain_kind = chain_kind_of(s);
    p.n_steps = two ? 3 : 2;
    // two heads: each head's tail runs ITS half of the last entry GEMM (the concatenation YY is then never written)
    const bool halves = two && half_entry_form(s.c_in_phys(2), s.cs, s.os) && chain_flow_form(s, 0);
    bool entry_done = false;
    for (int i = 0; i < p.n_steps; ++i) {
        VortexStep &v = p.step[i];
        const bool last = i == p.n_steps - 1;
        v.vortex = last ? 2 : two ? 1 - i : 0;
        v.set = v.vortex == 1 ? 1 : 0;
        v.chain_flow = chain_flow_form(s, v.vortex);
        v.entry_ntin = entry_tiles(s.c_in_phys(v.vortex), s.cs);
        v.entry = !v.chain_flow ? ENTRY_GENERIC : (last && entry_done) ? ENTRY_BY_PREV_TAIL : ENTRY_KERNEL;
        v.in_split = !last && p.dense == DENSE_CHAIN;
        v.split = h16 && v.chain_flow;
        v.z2 = last && halves;
        v.half = -1;
        v.branches = v.chain_flow || s.npix < 32768 ? BRANCH_GROUPED : BRANCH_GROUPED_SIDE0;  // (small frames: the stream hand-over costs more than it hides)
        if (!fused) v.tail = TAIL_UNFUSED;
        else if (last) v.tail = p.chain_kind ? TAIL_HEAD : TAIL_ALONE;
        else if (halves) { v.tail = TAIL_HALF_ENTRY; v.half = v.vortex; }
        // single head: this tail runs the last VortexPooling's entry GEMM on its register-resident result
        else if (!two && v.chain_flow && chain_flow_form(s, 2) && s.c_in_phys(2) == s.os) v.tail = TAIL_ENTRY;
        else v.tail = TAIL_ALONE;
        if (v.tail == TAIL_ENTRY || v.tail == TAIL_HALF_ENTRY) entry_done = true;
        if (v.in_split && (!v.chain_flow || v.entry != ENTRY_KERNEL)) return "internal error (split-plane input without the entry kernel)";
    }
    p.head_layers = p.step[p.n_steps - 1].tail != TAIL_HEAD;
    // (a net with a chain-form head - chain_kind - has fused tails, and the last one runs the head)
    if (p.chain_kind && p.head_layers) return "internal error (the last tail did not run the prediction head)";
    return nullptr;
}

// The launches of a planned pass in host enqueue order (what ojf_net_profile reports for it)
static std::vector<Launch> plan_launches(const NetShape &s, const ForwardPlan &p)
{
    std::vector<Launch> out;
    const Launch conv1 = conv_launch(s.arith, 1);
    for (int i = 0; i < p.n_steps; ++i) {
        const VortexStep &v = p.step[i];
        if (v.vortex < 2) {
            if (p.dense == DENSE_CHAIN) out.push_back(L_DENSE_CHAIN);
            else if (p.dense == DENSE_PAIRS) out.insert(out.end(), s.gf, L_DENSE_PAIR);
            else out.insert(out.end(), 2 * s.gf, conv1);
        }
        if (v.entry == ENTRY_GENERIC) out.insert(out.end(), {L_COLSUM, L_GAVE_BIAS, conv1});
        else if (v.entry == ENTRY_KERNEL) out.push_back(L_ENTRY1X1);
        out.push_back(L_POOL_PYRAMID);
        switch (v.branches) {
        case BRANCH_GROUPED: out.insert(out.end(), 2, conv_launch(s.arith, 4)); break;
        case BRANCH_GROUPED_SIDE0: out.insert(out.end(), 2, conv1); out.insert(out.end(), 2, conv_launch(s.arith, 3)); break;
        }
        switch (v.tail) {
        case TAIL_UNFUSED: out.insert(out.end(), 5, conv1); break;
        case TAIL_ALONE: out.push_back(L_TAIL); break;
        case TAIL_ENTRY: out.push_back(L_TAIL_ENTRY); break;
        case TAIL_HALF_ENTRY: out.push_back(L_TAIL_HALF_ENTRY); break;
        case TAIL_HEAD: out.push_back(L_TAIL_HEAD); break;
        }
    }
    if (p.head_layers) out.insert(out.end(), 2 * (s.gf - 1) + 3, conv1);
    return out;
}

struct Vortex {
    int c_in = 0, c_in_phys = 0;
    PackedConv stacked, b3a[4], b3b[4], b1[4], fin;
    float *pool_bias[4] = {nullptr, nullptr, nullptr, nullptr};
    float *Wg = nullptr, *bg = nullptr, *Wfg = nullptr, *bf = nullptr, *bias_final = nullptr;
    float *tail_w = nullptr, *tail_b1 = nullptr, *tail_rinv = nullptr;  // fused tail (closing 1x1s + final conv), when supported
    float *entry_w = nullptr, *entry_b = nullptr;  // the stacked entry GEMM as one chain layer (entry_tiles() input tiles -> 5), when supported
    // two-head nets (round 6): the last VortexPooling's entry GEMM over the concatenation of the two heads' outputs splits into
    // one 8-tile -> 5 layer per head (columns [hd * os, (hd + 1) * os) of the stacked weights, no bias, no activation): each head's
    // tail runs ITS half on its register-resident result; the pool pyramid adds the halves (and forms branch 0)
    float *entry_wh[2] = {nullptr, nullptr}, *entry_bh[2] = {nullptr, nullptr}, *bias0 = nullptr;
};

}  // namespace ojf

struct ojf_net {
    int version, P, c, cs, gf, sem, heads, h, w, npix;
    int arith;  // OJF_ARITH_* captured at creation
    ojf::NetShape shape;    // the same, as the planner and the packing predicates read it
    ojf::ForwardPlan plan;  // the launches of a forward pass, decided in ojf_net_create (plan_forward)
    int pool_in, os;  // (gf+1)*c and its padded slot
    float scale;
    int64_t macs_per_pixel;
    int last_launches = 0;  // kernel launches of the most recent ojf_net_forward (all streams)
    std::vector<ojf::PackedConv> dense[2];  // block0 / block2 (or v2's block): 2*gf convs each
    std::vector<ojf::PackedPair> pairs[2];  // split-fp16: the same layers packed for dense_pair_kernel (one launch per Block)
    ojf::PackedChain chains[2];             // ... and for dense_chain_kernel (all Blocks of a head in one launch; X[] then hold split planes)
    ojf::Vortex vortex[3];                  // v3: vortex0, vortex2, vortex3 ; v2: vortex, -, vortex_final
    std::vector<ojf::PackedConv> pred;
    float *chain_w = nullptr, *chain_b = nullptr;  // fused prediction head (plan.chain_kind: 19 / 20 growth channels)
    // activation planes (C4 layout), sizes in channels
    float *X[2] = {nullptr, nullptr};  // dense-growth buffers, (gf+1)*cs
    // Scratch of one head's dense block + VortexPooling.  Two sets: with two heads (v3 + semantics) the second head runs
    // concurrently on its own stream (the kernels are latency-bound and leave most of the GPU idle), so it needs its
    // own intermediates, side stream and events; everything else (and the last VortexPooling) uses set 0.
    struct Scratch {
        float *T = nullptr, *Z = nullptr, *Q1 = nullptr, *Q2 = nullptr, *Q3 = nullptr, *U = nullptr, *V = nullptr;
        float *Q0 = nullptr;  // two-head nets: branch 0 of the last VortexPooling (the pyramid's level-0 pass)
        float *partial = nullptr;
        ojf::ColSums *colsum = nullptr;  // chain flow: fixed-point channel sums of the entry layer's input (zero between frames)
        float *CAT = nullptr;  // 4*os, unfused tail only (allocated when the plan has one on this set)
        hipStream_t side = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_entry = nullptr;
    } sc[2];
    hipStream_t head1 = nullptr;  // stream of the second head
    hipStream_t head_paired_with = nullptr;  // launch stream head1 was tested against (pair_head_stream)
    bool head_paired = false;
    hipEvent_t ev_head_fork = nullptr, ev_head_join = nullptr;
    // (per set: T cs | Z 4*cs entry-conv output | Q1..Q3 cs pool-pyramid outputs | U, V 4*cs outputs of the branches'
    //  first / closing 3x3 | partial kSumBlocks*256 | side stream + events of the global-average branch)
    // two-head nets: the channel sums of the LAST VortexPooling's input come from the two heads' tails, which run on two streams beside
    // the first head's own VortexPooling - whose pyramid reads and zeroes sc[0].colsum: they need an accumulator of their own
    ojf::ColSums *colsum3 = nullptr;
    float *YY = nullptr;               // heads*os (vortex0 | vortex2 outputs)
    float *Y3 = nullptr;               // os
    float *PA = nullptr, *PB = nullptr;  // pred ping-pong, os each (allocated when the plan runs the head layer by layer)
    // Optional (OJF_NET_GRAPH=1): the launch sequence of a forward pass captured once per output buffer and
    // replayed with hipGraphLaunch.  Measured on ROCm 7.2 / MI355X: host enqueue time of a forward 160 -> 87 us,
    // but the GPU runs the graph 3-8 % SLOWER than the plain launches (0.555 vs 0.538 ms at 320x240,
    // 0.293 vs 0.270 ms at 160x120), and the host (0.21 ms/frame in Pipeline.fuse) is not the bound: off by default.
    hipStream_t cap = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    float *g_est = nullptr;
    int g_stride = 0;
    bool use_graph = false;
};

namespace ojf {

// every activation buffer keeps kPrefix floats of zeros in front of its planes: index -1 (in float4
// units) is what out-of-image taps read
constexpr size_t kPrefix = 64;  // keeps the planes 256-byte aligned

static int alloc_planes(float **p, size_t npix, int ch)
{
    float *raw = nullptr;
    OJF_HIP(hipMalloc(reinterpret_cast<void **>(&raw), (npix * ch + kPrefix) * sizeof(float)));
    OJF_HIP(hipMemset(raw, 0, (npix * ch + kPrefix) * sizeof(float)));
    // The fill runs on the null stream; the second head's stream and the side streams are hipStreamNonBlocking and do NOT
    // order against it: a convolution on such a stream could write the buffer before the fill zeroes it (round 5, when the
    // fall-back buffers were still allocated inside a forward pass: one wrong output in ~8 suite runs of the generic two-head
    // topology, never in isolation).  The fill is therefore complete before anybody learns the pointer.
    OJF_HIP(hipStreamSynchronize(nullptr));
    *p = raw + kPrefix;
    return 0;
}

static void free_planes(float *p)
{
    if (p) (void)hipFree(p - kPrefix);
}

static int build_vortex(ojf_net *net, int k, const ojf_conv_layer *L, int c_in, const std::vector<int> &in_map)
{
    Vortex &v = net->vortex[k];
    const int c_in_phys = net->shape.c_in_phys(k);
    // L[0] gave 1x1 | L[1+4b .. 4+4b] branch b: 1x1, 3x3, 3x3, 1x1 | L[17] final 1x1 (5*out -> out)
    const int c = net->c, cs = net->cs, out = net->pool_in, os = net->os;
    v.c_in = c_in;
    v.c_in_phys = c_in_phys;
    for (int i = 0; i < 18; ++i) {
        const bool k3 = (i >= 1 && i <= 16) && ((i - 1) % 4 == 1 || (i - 1) % 4 == 2);
        if (L[i].ksize != (k3 ? 3 : 1)) return fail("ojf_net_create: unexpected kernel size in a VortexPooling layer");
    }
    if (L[0].c_in != c_in || L[0].c_out != out || L[17].c_in != 5 * out || L[17].c_out != out)
        return fail("ojf_net_create: VortexPooling layer shapes do not match the topology");
    {   // stacked branch-entry 1x1: c_in -> 4 slots of cs; only branch 0 gets its bias (+ReLU) here
        ConvBuilder b(c_in_phys, 4 * cs, 1, 1);
        for (int br = 0; br < 4; ++br) {
            const ojf_conv_layer &l = L[1 + 4 * br];
            if (l.c_in != c_in || l.c_out != c) return fail("ojf_net_create: branch entry conv shape mismatch");
            b.add(l, 0, c_in, in_map, br * cs, br == 0);
            if (br > 0) {
                std::vector<float> pb(cs, 0.0f);
                for (int o = 0; o < c; ++o) pb[o] = l.bias_host[o];
                if (upload(pb, &v.pool_bias[br])) return -2;
            }
        }
        if (finish(b, v.stacked, net->arith)) return -2;
        if (const int ntin = entry_tiles(c_in_phys, cs)) {
            // chain-layer form (entry1x1_kernel / the previous tail): 8 input tiles -> 5; the two-head net's last VortexPooling
            // (228 = 2 x 114 input channels): 16 -> 5 (round 6: it ran the generic convolution + two side-stream kernels + three events)
            auto we = [&](int oc, int k) { return oc < 4 * cs && k < c_in_phys ? b.W[(size_t)oc * c_in_phys + k] : 0.0f; };
            const std::vector<float> re = chain_row_scales(net->arith, 5, c_in_phys, we);
            std::vector<float> ew, eb;
            pack_chain_layer(ew, net->arith, 5, ntin, re, we);
            append_chain_bias(eb, net->arith, 5, 4 * cs, b.B.data(), re);
            if (upload(ew, &v.entry_w) || upload(eb, &v.entry_b)) return -2;
            if (half_entry_form(c_in_phys, cs, os)) {
                const std::vector<float> zero_bias(4 * cs, 0.0f);
                for (int hd = 0; hd < 2; ++hd) {
                    auto wh = [&](int oc, int k) { return oc < 4 * cs && k < net->os ? b.W[(size_t)oc * c_in_phys + hd * net->os + k] : 0.0f; };
                    const std::vector<float> rh = chain_row_scales(net->arith, 5, net->os, wh);
                    std::vector<float> hw, hb;
                    pack_chain_layer(hw, net->arith, 5, 8, rh, wh);
                    append_chain_bias(hb, net->arith, 5, 4 * cs, zero_bias.data(), rh);
                    if (upload(hw, &v.entry_wh[hd]) || upload(hb, &v.entry_bh[hd])) return -2;
                }
                std::vector<float> b0(cs, 0.0f);
                for (int o = 0; o < cs; ++o) b0[o] = b.B[o];  // branch 0's bias (+ ReLU): applied by the pyramid's level-0 pass
                if (upload(b0, &v.bias0)) return -2;
            }
        }
    }
    const std::vector<int> id_c = slot_map(c, c, cs);
    for (int br = 0; br < 4; ++br) {
        const ojf_conv_layer &la = L[2 + 4 * br], &lb = L[3 + 4 * br], &l1 = L[4 + 4 * br];
        if (la.c_in != c || la.c_out != c || lb.c_in != c || lb.c_out != c || l1.c_in != c || l1.c_out != out)
            return fail("ojf_net_create: branch conv shape mismatch");
        ConvBuilder ba(cs, cs, 3, la.dilation), bb(cs, cs, 3, lb.dilation), b1(cs, os, 1, 1);
        ba.add(la, 0, c, id_c, 0, true);
        bb.add(lb, 0, c, id_c, 0, true);
        b1.add(l1, 0, c, id_c, 0, true);
        if (finish(ba, v.b3a[br], net->arith) || finish(bb, v.b3b[br], net->arith) || finish(b1, v.b1[br], net->arith)) return -2;
    }
    {   // final 1x1 over [gave | b0 | b1 | b2 | b3]; the gave columns become a per-frame bias
        const ojf_conv_layer &lf = L[17];
        ConvBuilder b(4 * os, os, 1, 1);
        b.add(lf, out, 5 * out, slot_map(4 * out, out, os), 0, false);
        if (finish(b, v.fin, net->arith)) return -2;
        // (the two matrices rounded up to whole float4: gave_bias_block streams them as flat 16-byte loads)
        std::vector<float> Wg(((size_t)out * c_in_phys + 3) / 4 * 4, 0.0f), bg(out), Wfg(((size_t)out * out + 3) / 4 * 4, 0.0f), bf(out);
        for (int o = 0; o < out; ++o) {  // stored transposed: [input][output]
            for (int ci = 0; ci < c_in; ++ci) Wg[(size_t)in_map[ci] * out + o] = L[0].weight_host[(size_t)o * c_in + ci];
            bg[o] = L[0].bias_host[o];
            for (int j = 0; j < out; ++j) Wfg[(size_t)j * out + o] = lf.weight_host[(size_t)o * 5 * out + j];
            bf[o] = lf.bias_host[o];
        }
        if (upload(Wg, &v.Wg) || upload(bg, &v.bg) || upload(Wfg, &v.Wfg) || upload(bf, &v.bf)) return -2;
        std::vector<float> zero((size_t)v.fin.n_ot * 16, 0.0f);
        if (upload(zero, &v.bias_final)) return -2;
    }
    if (fused_tail_form(cs, os)) {  // fused tail: [W1_b | Wf_b] fragments per branch
        const int NV = 2, NO = 8;
        std::vector<float> tw, tb;
        const ojf_conv_layer &lf = L[17];
        // the four column blocks of the final conv accumulate into one set of rows: one common row scale
        const std::vector<float> rf = chain_row_scales(net->arith, NO, 4 * out, [&](int oc, int k) {
            return oc < out ? lf.weight_host[(size_t)oc * 5 * out + out + k] : 0.0f;
        });
        for (int br = 0; br < 4; ++br) {
            const ojf_conv_layer &l1 = L[4 + 4 * br];
            auto w1 = [&](int oc, int k) { return oc < out && k < c ? l1.weight_host[(size_t)oc * c + k] : 0.0f; };
            const std::vector<float> r1 = chain_row_scales(net->arith, NO, c, w1);
            pack_chain_layer(tw, net->arith, NO, NV, r1, w1);
            pack_chain_layer(tw, net->arith, NO, NO, rf, [&](int oc, int k) {
                return oc < out && k < out ? lf.weight_host[(size_t)oc * 5 * out + out * (br + 1) + k] : 0.0f;
            });
            append_chain_bias(tb, net->arith, NO, out, l1.bias_host, r1);
        }
        std::vector<float> rfi(rf.size());
        for (size_t i = 0; i < rf.size(); ++i) rfi[i] = 1.0f / rf[i];
        if (upload(rfi, &v.tail_rinv)) return -2;
        if (upload(tw, &v.tail_w) || upload(tb, &v.tail_b1)) return -2;
    }
    return 0;
}

static void free_vortex(Vortex &v)
{
    release(v.stacked);
    release(v.fin);
    for (int b = 0; b < 4; ++b) {
        release(v.b3a[b]);
        release(v.b3b[b]);
        release(v.b1[b]);
        if (v.pool_bias[b]) (void)hipFree(v.pool_bias[b]);
    }
    float *ptrs[] = {v.Wg, v.bg, v.Wfg, v.bf, v.bias_final, v.tail_w, v.tail_b1, v.tail_rinv, v.entry_w, v.entry_b,
                     v.entry_wh[0], v.entry_wh[1], v.entry_bh[0], v.entry_bh[1], v.bias0};
    for (float *p : ptrs)
        if (p) (void)hipFree(p);
}

// in: planes, window starting at group in_g0 (c_in_phys/4 groups); out: planes at group out_g0
static GaveArgs gave_args(const ojf_net *net, const Vortex &v, const float *partial, int nparts, int pstride, ColSums *fixed = nullptr)
{
    GaveArgs ga;
    ga.partial = partial; ga.fixed = fixed; ga.nparts = nparts; ga.pstride = pstride; ga.cphys = v.c_in_phys; ga.npix = net->npix;
    ga.WgT = v.Wg; ga.bg = v.bg; ga.WfgT = v.Wfg; ga.bf = v.bf; ga.c_out = net->pool_in;
    ga.bias_out = v.bias_final; ga.bias_len = v.fin.n_ot * 16;
    return ga;
}

// The pool pyramid launch of filled arguments (h, w, c4, fold_gave, z2 set; tiles is derived here).  grid.x: the tiles (+ the
// global-average block of the chain flow) rounded up to a multiple of 8 (XCD bands); grid.y: three branches' groups, four with z2
static dim3 launch_pyramid(PyramidArgs &pa, hipStream_t st)
{
    pa.tiles = ((pa.w + kPoolTW - 1) / kPoolTW) * ((pa.h + kPoolTH - 1) / kPoolTH);
    const dim3 pgrid(round_up(pa.tiles + (pa.fold_gave ? 1 : 0), 8), (pa.z2 ? 4 : 3) * pa.c4);
    hipLaunchKernelGGL(pool_pyramid_kernel, pgrid, dim3(256), 0, st, pa);
    return pgrid;
}

static int chain_blocks(const ojf_net *net) { return ((net->npix + 15) / 16 + ojf::kChainWaves - 1) / ojf::kChainWaves; }  // blocks of the MT = 1 chain kernels

// The persistent entry GEMM over `strips` 64-pixel strips: min(strips, kChainBlocks x CUs) blocks - what the device holds at once,
// though nothing depends on it - or at most max_blocks of them (> 0: tests, so that a tiny frame walks several strips per block).
static void launch_entry_persistent(const ChainArgs &ea, int strips, int max_blocks, hipStream_t st)
{
    const int cus = device_cu_count();
    int blocks = cus > 0 && ojf::kChainBlocks * cus < strips ? ojf::kChainBlocks * cus : strips;
    if (max_blocks > 0 && max_blocks < blocks) blocks = max_blocks;
    if (ea.in_split) hipLaunchKernelGGL(entry1x1_persistent_kernel<true>, dim3(blocks), dim3(ojf::kChainThreads), 0, st, ea, strips);
    else hipLaunchKernelGGL(entry1x1_persistent_kernel<false>, dim3(blocks), dim3(ojf::kChainThreads), 0, st, ea, strips);
}

// one launch of a chain-layer kernel template in the net's arithmetic: KERNEL<arithmetic, further template arguments>(ARGS)
#define OJF_LAUNCH_BY_ARITH(KERNEL, ARGS, ...)                                                                              \
    do {                                                                                                                     \
        if (h16) hipLaunchKernelGGL((KERNEL<OJF_ARITH_F16X3, __VA_ARGS__>), grid, block, 0, st, ARGS);                      \
        else hipLaunchKernelGGL((KERNEL<OJF_ARITH_F32, __VA_ARGS__>), grid, block, 0, st, ARGS);                            \
    } while (0)

// One VortexPooling as its step of the plan says.  Steps 0 / 1 read their head's dense-growth buffer and write (where the tail
// carries nothing along) their slot of YY; the last one reads YY and writes Y3.  `head`: the prediction head's arguments, for
// the tail that runs it.
#ifdef OJF_TAIL_STAMPS  // profiling build only: which form of the two headline tails the forward pass launches (tools/tail_stamps.py)
static int g_tail_stamp_form = ojf::kTailNext;
static int tail_stamp_form() { return g_tail_stamp_form; }
#endif

static int run_vortex(ojf_net *net, const VortexStep &s, hipStream_t st, const ChainArgs &head)
{
    const int h = net->h, w = net->w, c4 = net->cs / 4, o4 = net->os / 4;
    const bool h16 = net->arith == OJF_ARITH_F16X3;
    const bool last = s.vortex == 2;
    const Vortex &v = net->vortex[s.vortex], &next = net->vortex[2];
    ojf_net::Scratch &sc = net->sc[s.set];
    const float *in = last ? net->YY : net->X[s.vortex];
    float *out = last ? net->Y3 : net->YY;
    const int in_g0 = 0, out_g0 = last ? 0 : s.vortex * o4;
    const dim3 grid(chain_blocks(net)), block(ojf::kChainThreads);
    const int banded = (grid.x & 7) == 0 ? 1 : 0;  // (banded_block_x; for the trace only)

    // ---- entry: the four branch-entry 1x1 as one GEMM into sc.Z, the global-average branch's column sums ----------------
    if (s.entry == ENTRY_GENERIC) {
        // global-average branch -> bias of the final conv, on the side stream (fork here, join before the tail)
        OJF_HIP(hipEventRecord(sc.ev_fork, st));
        OJF_HIP(hipStreamWaitEvent(sc.side, sc.ev_fork, 0));
        const dim3 sgrid(kSumBlocks, v.c_in_phys / 4), ggrid(1);
        hipLaunchKernelGGL(colsum_kernel, sgrid, dim3(256), 0, sc.side, planes(in), in_g0, net->npix, sc.partial);
        if (net_trace_on()) fprintf(stderr, "ojf_net %s | grid_x %u grid_y %u\n", kLaunchNames[L_COLSUM], sgrid.x, sgrid.y);
        mark_launch(L_COLSUM, sc.side);
        OJF_HIP(hipGetLastError());
        hipLaunchKernelGGL(gave_bias_kernel, ggrid, dim3(256), 0, sc.side, gave_args(net, v, sc.partial, kSumBlocks, 256));
        if (net_trace_on()) fprintf(stderr, "ojf_net %s | grid_x %u grid_y %u\n", kLaunchNames[L_GAVE_BIAS], ggrid.x, ggrid.y);
        mark_launch(L_GAVE_BIAS, sc.side);
        OJF_HIP(hipGetLastError());
        // branch entries: one GEMM, branch 0 gets bias + ReLU in the epilogue
        if (launch_conv(v.stacked, in, in_g0, sc.Z, 0, nullptr, OJF_ACT_RELU, net->cs, 1.0f, h, w, st)) return -2;
        OJF_HIP(hipEventRecord(sc.ev_entry, st));
    } else if (s.entry == ENTRY_KERNEL) {
        ChainArgs ea;
        ea.in = planes(in); ea.w = planes(v.entry_w); ea.bias = v.entry_b; ea.out_rows = nullptr;
        ea.in_g0 = in_g0; ea.c4_in = v.c_in_phys / 4; ea.npix = net->npix; ea.rows_stride = 0; ea.rows_n = 0; ea.scale = 1.0f;
        ea.ovf = h16 ? overflow_flag() : nullptr;
        ea.out_planes = planes(sc.Z); ea.out_g0 = 0; ea.og_store = 4 * c4; ea.act_n = net->cs; ea.colsum = sc.colsum;
        ea.split_groups = s.split ? c4 : 0;
        ea.in_split = s.in_split ? 1 : 0;
#ifdef OJF_ENTRY_STAMPS
        ea.stamp = 1;
#endif
        // (two pixel tiles per wave - half the blocks, half the weight stream per pixel - measured 22.2 against 23.7 us and changes the
        // rounding of the channel sums: not kept, profiles/r06_fusion_net_experiments.txt)
        if (s.entry_ntin == 16) OJF_LAUNCH_BY_ARITH(entry1x1_kernel, ea, 1, 16, 5);
        else if (h16) launch_entry_persistent(ea, (int)grid.x, 0, st);  // (profiles/entry_gemm_persistent.txt)
        else OJF_LAUNCH_BY_ARITH(entry1x1_kernel, ea, 1, 8, 5);
        if (net_trace_on())
            fprintf(stderr, "ojf_net %s | ntin %d blocks %u banded %d\n", kLaunchNames[L_ENTRY1X1], s.entry_ntin, grid.x, banded);
        mark_launch(L_ENTRY1X1, st);
        OJF_HIP(hipGetLastError());
    }

    // ---- branches: pool pyramid, then the dilated 3x3 pair of each of the four branches into sc.V -------------------------
    {   // pool pyramid on the pre-activations of branches 1..3: Q_b = ReLU(pool^b(Z[slot b]) + bias_b), one launch
        PyramidArgs pa;
        pa.z = planes(sc.Z);
        pa.q[0] = planes(sc.Q1); pa.q[1] = planes(sc.Q2); pa.q[2] = planes(sc.Q3);
        for (int b = 0; b < 3; ++b) pa.bias[b] = v.pool_bias[b + 1];
        pa.h = h; pa.w = w; pa.c4 = c4;
        pa.gave = gave_args(net, v, nullptr, 0, 0, s.z2 ? net->colsum3 : sc.colsum);
        pa.fold_gave = s.chain_flow ? 1 : 0;
        pa.split_out = s.split ? 1 : 0;
        if (s.z2) { pa.z2 = planes(net->sc[1].Z); pa.q0 = planes(sc.Q0); pa.bias0 = v.bias0; }
        const dim3 pgrid = launch_pyramid(pa, st);
        if (net_trace_on()) fprintf(stderr, "ojf_net %s | tiles %d grid_x %u grid_y %u\n", kLaunchNames[L_POOL_PYRAMID], pa.tiles, pgrid.x, pgrid.y);
        mark_launch(L_POOL_PYRAMID, st);
        OJF_HIP(hipGetLastError());
    }
    const float *bin[4] = {s.z2 ? sc.Q0 : sc.Z, sc.Q1, sc.Q2, sc.Q3};
    {   // the four branches' dilated 3x3 pairs: two grouped launches (all first convs, then all second convs)
        ConvArgs ga[4], gb[4];
        for (int br = 0; br < 4; ++br) {
            fill_conv_args(ga[br], v.b3a[br], bin[br], 0, sc.U, br * c4, nullptr, OJF_ACT_RELU, net->cs, 1.0f, h, w);
            fill_conv_args(gb[br], v.b3b[br], sc.U, br * c4, sc.V, br * c4, nullptr, OJF_ACT_RELU, net->cs, 1.0f, h, w);
            ga[br].in_split = ga[br].out_split = gb[br].in_split = s.split ? 1 : 0;
        }
        if (s.branches == BRANCH_GROUPED) {
            if (launch_conv_args(ga, 4, v.b3a[0].n_ot, st, net->arith)) return -2;
            if (launch_conv_args(gb, 4, v.b3b[0].n_ot, st, net->arith)) return -2;
        } else {  // BRANCH_GROUPED_SIDE0
            OJF_HIP(hipStreamWaitEvent(sc.side, sc.ev_entry, 0));
            if (launch_conv_args(ga, 1, v.b3a[0].n_ot, sc.side, net->arith)) return -2;
            if (launch_conv_args(gb, 1, v.b3b[0].n_ot, sc.side, net->arith)) return -2;
            if (launch_conv_args(ga + 1, 3, v.b3a[1].n_ot, st, net->arith)) return -2;
            if (launch_conv_args(gb + 1, 3, v.b3b[1].n_ot, st, net->arith)) return -2;
        }
    }

    // ---- tail: the four branch-exit 1x1, the final 1x1 over their concatenation (+ the global-average bias) ---------------
    if (!s.chain_flow) {
        OJF_HIP(hipEventRecord(sc.ev_join, sc.side));
        OJF_HIP(hipStreamWaitEvent(st, sc.ev_join, 0));  // bias of the final conv is ready
    }
    if (s.tail == TAIL_UNFUSED) {
        for (int br = 0; br < 4; ++br)
            if (launch_conv(v.b1[br], sc.V, br * c4, sc.CAT, br * o4, nullptr, OJF_ACT_RELU, net->os, 1.0f, h, w, st))
                return -2;
        return launch_conv(v.fin, sc.CAT, 0, out, out_g0, v.bias_final, OJF_ACT_NONE, 0, 1.0f, h, w, st);
    }
    // fused tail (the four branch-exit 1x1 and the final 1x1 in one launch), and what rides along with it
    TailArgs ta;
    for (int br = 0; br < 4; ++br) ta.v[br] = planes(sc.V) + (size_t)br * c4 * net->npix;
    ta.w = planes(v.tail_w); ta.b1 = v.tail_b1; ta.bias_final = v.bias_final; ta.rinv_final = v.tail_rinv;
    ta.out = planes(out); ta.c4 = c4; ta.out_g0 = out_g0; ta.og_store = o4; ta.npix = net->npix;
    ta.ovf = h16 ? overflow_flag() : nullptr;
    ta.chain_w = nullptr; ta.chain_b = nullptr; ta.out_rows = nullptr; ta.rows_stride = 0; ta.rows_n = 0; ta.scale = 1.0f;
    ta.entry_w = nullptr; ta.entry_b = nullptr; ta.entry_out = nullptr; ta.entry_og = 0; ta.entry_act_n = 0; ta.colsum = nullptr; ta.entry_split = 0;
    // MT = 1: two pixel tiles per wave (324 VGPRs, one wave per SIMD) measured slower (0.624 vs 0.609 ms net)
    Launch name = L_TAIL;
    switch (s.tail) {
    case TAIL_HEAD:  // last VortexPooling: the prediction head rides along
        name = L_TAIL_HEAD;
        ta.chain_w = head.w; ta.chain_b = head.bias; ta.out_rows = head.out_rows;
        ta.rows_stride = head.rows_stride; ta.rows_n = head.rows_n; ta.scale = head.scale;
#ifdef OJF_TAIL_STAMPS
        if (net->plan.chain_kind == 19 && h16 && tail_stamp_form() == ojf::kTailAtBranch)
            hipLaunchKernelGGL((vortex_tail_kernel<OJF_ARITH_F16X3, 1, 2, 8, 19, ojf::kTailAtBranch>), grid, block, 0, st, ta);
        else
#endif
        if (net->plan.chain_kind == 19) OJF_LAUNCH_BY_ARITH(vortex_tail_kernel, ta, 1, 2, 8, 19);
        else OJF_LAUNCH_BY_ARITH(vortex_tail_kernel, ta, 1, 2, 8, 20);
        break;
    case TAIL_HALF_ENTRY:
        name = L_TAIL_HALF_ENTRY;
        // two-head net: this head's HALF of the last VortexPooling's entry GEMM rides along (partial sums: no bias, no activation,
        // plain planes), the channel sums of its result go to colsum3 at channel half * os; `out` is never written
        ta.entry_w = planes(next.entry_wh[s.half]); ta.entry_b = next.entry_bh[s.half]; ta.entry_out = planes(sc.Z);
        ta.entry_og = 4 * c4; ta.entry_act_n = 0; ta.colsum = net->colsum3; ta.colsum_off = s.half * net->os;
        ta.entry_split = 0;
        OJF_LAUNCH_BY_ARITH(vortex_tail_kernel, ta, 1, 2, 8, kTailEntry);
        break;
    case TAIL_ENTRY:
        name = L_TAIL_ENTRY;
        // this VortexPooling feeds the last one: its entry GEMM and column sums ride along, `out` is never written
        ta.entry_w = planes(next.entry_w); ta.entry_b = next.entry_b; ta.entry_out = planes(sc.Z);
        ta.entry_og = 4 * c4; ta.entry_act_n = net->cs; ta.colsum = sc.colsum;
        ta.entry_split = h16 ? c4 : 0;  // (the last VortexPooling runs the chain flow: same rule as its `split`)
#ifdef OJF_TAIL_STAMPS
        if (h16 && tail_stamp_form() == ojf::kTailAtBranch)
            hipLaunchKernelGGL((vortex_tail_kernel<OJF_ARITH_F16X3, 1, 2, 8, kTailEntry, ojf::kTailAtBranch>), grid, block, 0, st, ta);
        else
#endif
        OJF_LAUNCH_BY_ARITH(vortex_tail_kernel, ta, 1, 2, 8, kTailEntry);
        break;
    default:  // TAIL_ALONE
        OJF_LAUNCH_BY_ARITH(vortex_tail_kernel, ta, 1, 2, 8);
        break;
    }
    if (net_trace_on()) fprintf(stderr, "ojf_net %s | blocks %u banded %d\n", kLaunchNames[name], grid.x, banded);
    mark_launch(name, st);
    return check_hip(hipGetLastError(), "vortex_tail_kernel launch");
}
#undef OJF_LAUNCH_BY_ARITH

static int run_dense(ojf_net *net, int head, hipStream_t st)
{
    const int c4 = net->cs / 4;
    float *T = net->sc[head].T;
    switch (net->plan.dense) {
    case DENSE_CHAIN: return launch_chain(net->chains[head], net->X[head], net->h, net->w, st);  // one launch (ojf_net_chain.h)
    case DENSE_PAIRS:  // one fused launch per Block (ojf_net_pair.h)
        for (int i = 0; i < net->gf; ++i)
            if (launch_pair(net->pairs[head][i], net->X[head], 0, net->X[head], (i + 1) * c4, net->h, net->w, st)) return -2;
        return 0;
    case DENSE_CONVS:
        for (int i = 0; i < net->gf; ++i) {
            if (launch_conv(net->dense[head][2 * i], net->X[head], 0, T, 0, nullptr, OJF_ACT_LEAKY, net->cs, 1.0f,
                            net->h, net->w, st)) return -2;
            if (launch_conv(net->dense[head][2 * i + 1], T, 0, net->X[head], (i + 1) * c4, nullptr, OJF_ACT_LEAKY,
                            net->cs, 1.0f, net->h, net->w, st)) return -2;
        }
        return 0;
    }
    return 0;
}

static int layer_count(int version, int gf, int sem)
{
    const int pred = 2 * (gf - 1) + 3;
    if (version == 3) return (sem ? 2 : 1) * (2 * gf + 18) + 18 + pred;
    if (version == 2) return 2 * gf + 18 + 18 + pred;
    return -1;
}

}  // namespace ojf

OJF_API int ojf_net_layer_count(int version, int n_points, int growth, int use_semantics)
{
    if (n_points < 1 || growth < 1) return -1;
    return ojf::layer_count(version, growth, use_semantics ? 1 : 0);
}

namespace ojf { static void drop_graph(ojf_net *net); }

OJF_API void ojf_net_destroy(ojf_net *net)
{
    using namespace ojf;
    if (!net) return;
    for (int hd = 0; hd < 2; ++hd) {
        for (auto &pc : net->dense[hd]) release(pc);
        for (auto &pp : net->pairs[hd]) release(pp);
        release(net->chains[hd]);
    }
    for (auto &pc : net->pred) release(pc);
    for (auto &v : net->vortex) free_vortex(v);
    float *bufs[] = {net->X[0], net->X[1], net->YY, net->Y3, net->PA, net->PB};
    for (float *p : bufs) free_planes(p);
    for (auto &sc : net->sc) {
        float *sb[] = {sc.T, sc.Z, sc.Q0, sc.Q1, sc.Q2, sc.Q3, sc.U, sc.V, sc.partial, sc.CAT};
        if (sc.colsum) (void)hipFree(sc.colsum);
        for (float *p : sb) free_planes(p);
        if (sc.ev_fork) (void)hipEventDestroy(sc.ev_fork);
        if (sc.ev_join) (void)hipEventDestroy(sc.ev_join);
        if (sc.ev_entry) (void)hipEventDestroy(sc.ev_entry);
        if (sc.side) (void)hipStreamDestroy(sc.side);
    }
    if (net->colsum3) (void)hipFree(net->colsum3);
    if (net->ev_head_fork) (void)hipEventDestroy(net->ev_head_fork);
    if (net->ev_head_join) (void)hipEventDestroy(net->ev_head_join);
    if (net->head1) (void)hipStreamDestroy(net->head1);
    drop_graph(net);
    if (net->cap) (void)hipStreamDestroy(net->cap);
    if (net->chain_w) (void)hipFree(net->chain_w);
    if (net->chain_b) (void)hipFree(net->chain_b);
    delete net;
}

OJF_API int ojf_net_create(ojf_net **out, int version, int n_points, int growth, int use_semantics, float output_scale,
                           const ojf_conv_layer *L, int n_layers, int h, int w)
{
    using namespace ojf;
    if (!out || !L) return fail("ojf_net_create: null pointer argument");
    *out = nullptr;
    NetShape shape;
    if (const char *why = net_shape(shape, version, n_points, growth, use_semantics, h, w, g_default_arith)) return refuse("ojf_net_create", why);
    const int sem = shape.sem;
    if (n_layers != layer_count(version, growth, sem)) return fail("ojf_net_create: wrong number of folded layers");
    for (int i = 0; i < n_layers; ++i)
        if (!L[i].weight_host || !L[i].bias_host || (L[i].ksize != 1 && L[i].ksize != 3) || L[i].dilation < 1)
            return fail("ojf_net_create: malformed layer descriptor");
    for (int i = 0; i < n_layers; ++i) {  // the split-fp16 range guard relies on finite parameters
        const size_t nw = (size_t)L[i].c_out * L[i].c_in * L[i].ksize * L[i].ksize;
        for (size_t k = 0; k < nw; ++k)
            if (!std::isfinite(L[i].weight_host[k])) return fail("ojf_net_create: non-finite weight");
        for (int k = 0; k < L[i].c_out; ++k)
            if (!std::isfinite(L[i].bias_host[k])) return fail("ojf_net_create: non-finite bias");
    }

    ForwardPlan plan;
    if (const char *why = plan_forward(shape, &plan)) return refuse("ojf_net_create", why);

    ojf_net *net = new ojf_net();
    net->shape = shape; net->plan = plan;
    net->version = version; net->P = n_points; net->gf = growth; net->sem = sem;
    net->arith = shape.arith;
    net->c = shape.c; net->cs = shape.cs; net->heads = shape.heads;
    net->h = h; net->w = w; net->npix = shape.npix;
    net->pool_in = shape.pool_in; net->os = shape.os;
    net->scale = output_scale;
    const int c = net->c, cs = net->cs, gf = growth, os = net->os;
    net->macs_per_pixel = 0;
    for (int i = 0; i < n_layers; ++i) net->macs_per_pixel += (int64_t)L[i].c_in * L[i].c_out * L[i].ksize * L[i].ksize;

    int rc = 0;
    int li = 0;
    auto build_dense = [&](int head) -> int {
        std::vector<ConvBuilder> bas, bbs;
        for (int i = 0; i < gf; ++i) {
            const ojf_conv_layer &la = L[li++], &lb = L[li++];
            if (la.ksize != 3 || lb.ksize != 3 || la.c_in != (i + 1) * c || la.c_out != c || lb.c_in != c || lb.c_out != c)
                return fail("ojf_net_create: dense block layer shape mismatch");
            ConvBuilder ba((i + 1) * cs, cs, 3, la.dilation), bb(cs, cs, 3, lb.dilation);
            ba.add(la, 0, (i + 1) * c, slot_map((i + 1) * c, c, cs), 0, true);
            bb.add(lb, 0, c, slot_map(c, c, cs), 0, true);
            PackedConv pa, pb;
            if (finish(ba, pa, net->arith) || finish(bb, pb, net->arith)) return -2;
            net->dense[head].push_back(pa);
            net->dense[head].push_back(pb);
            if (pair_form(shape)) {
                PackedPair pp;
                if (finish_pair(ba, bb, pp, pair_cfg_for(net->h, net->w))) return -2;
                net->pairs[head].push_back(pp);
                bas.push_back(ba);
                bbs.push_back(bb);
            }
        }
        if (chain_form(shape) && finish_chain(bas, bbs, net->chains[head])) return -2;
        return 0;
    };
    const std::vector<int> dense_map = slot_map(net->pool_in, c, cs);
    const std::vector<int> flat_map = slot_map(net->pool_in, net->pool_in, os);
    if (version == 3) {
        rc = build_dense(0);
        if (!rc) { rc = build_vortex(net, 0, L + li, net->pool_in, dense_map); li += 18; }
        if (!rc && sem) {
            rc = build_dense(1);
            if (!rc) { rc = build_vortex(net, 1, L + li, net->pool_in, dense_map); li += 18; }
        }
        if (!rc) {
            rc = build_vortex(net, 2, L + li, net->heads * net->pool_in, slot_map(net->heads * net->pool_in, net->pool_in, os));
            li += 18;
        }
    } else {
        rc = build_dense(0);
        if (!rc) { rc = build_vortex(net, 0, L + li, net->pool_in, dense_map); li += 18; }
        if (!rc) { rc = build_vortex(net, 2, L + li, net->pool_in, flat_map); li += 18; }
    }
    if (!rc) {
        int prev_phys = os;
        for (; li < n_layers; ++li) {
            const ojf_conv_layer &l = L[li];
            if (l.ksize != 1) { rc = fail("ojf_net_create: prediction head must be 1x1 convolutions"); break; }
            if (round_up(l.c_in, 4) != prev_phys) { rc = fail("ojf_net_create: prediction head shapes do not chain"); break; }
            ConvBuilder b(prev_phys, round_up(l.c_out, 4), 1, 1);
            b.add(l, 0, l.c_in, slot_map(l.c_in, l.c_in, prev_phys), 0, true);
            PackedConv pc;
            if (finish(b, pc, net->arith)) { rc = -2; break; }
            net->pred.push_back(pc);
            prev_phys = round_up(l.c_out, 4);
        }
    }
    if (!rc && plan.chain_kind) {
        // fused prediction head: repack the 11 pointwise layers as chain_layer fragments
        const int first = n_layers - (2 * (gf - 1) + 3);
        std::vector<float> cw, cb;
        int prev_phys = os;
        for (int l = first; l < n_layers; ++l) {
            const ojf_conv_layer &ly = L[l];
            const int nt_in = (prev_phys + 15) / 16, out_phys = round_up(ly.c_out, 4), nt_out = (out_phys + 15) / 16;
            auto wl = [&](int oc, int k) { return oc < ly.c_out && k < ly.c_in ? ly.weight_host[(size_t)oc * ly.c_in + k] : 0.0f; };
            const std::vector<float> rs = chain_row_scales(net->arith, nt_out, ly.c_in, wl);
            pack_chain_layer(cw, net->arith, nt_out, nt_in, rs, wl);
            append_chain_bias(cb, net->arith, nt_out, ly.c_out, ly.bias_host, rs);
            prev_phys = out_phys;
        }
        if (upload(cw, &net->chain_w) || upload(cb, &net->chain_b)) rc = -2;
    }
    if (!rc) {  // the gave convs act on a 1x1 map: not a per-pixel cost
        int idx = 0;
        auto skip_dense = [&]() { idx += 2 * gf; };
        auto sub_gave = [&]() { net->macs_per_pixel -= (int64_t)L[idx].c_in * L[idx].c_out; idx += 18; };
        skip_dense(); sub_gave();
        if (version == 3 && sem) { skip_dense(); sub_gave(); }
        sub_gave();
    }
    const size_t np = (size_t)net->npix;
    if (!rc) rc = alloc_planes(&net->X[0], np, (gf + 1) * cs);
    if (!rc && net->heads == 2) rc = alloc_planes(&net->X[1], np, (gf + 1) * cs);
    for (int hd = 0; hd < net->heads && !rc; ++hd) {
        ojf_net::Scratch &sc = net->sc[hd];
        rc = alloc_planes(&sc.T, np, cs);
        if (!rc) rc = alloc_planes(&sc.Z, np, 4 * cs);
        if (!rc && hd == 0 && net->heads == 2) rc = alloc_planes(&sc.Q0, np, cs);
        if (!rc) rc = alloc_planes(&sc.Q1, np, cs);
        if (!rc) rc = alloc_planes(&sc.Q2, np, cs);
        if (!rc) rc = alloc_planes(&sc.Q3, np, cs);
        if (!rc) rc = alloc_planes(&sc.U, np, 4 * cs);
        if (!rc) rc = alloc_planes(&sc.V, np, 4 * cs);
        if (!rc) rc = alloc_planes(&sc.partial, kSumBlocks, 256);
        for (int i = 0; i < plan.n_steps && !rc; ++i)  // fall-back buffer of the unfused tail
            if (plan.step[i].set == hd && plan.step[i].tail == TAIL_UNFUSED && !sc.CAT) rc = alloc_planes(&sc.CAT, np, 4 * os);
        if (!rc) rc = check_hip(hipMalloc(reinterpret_cast<void **>(&sc.colsum), sizeof(ColSums)), "hipMalloc");
        if (!rc) rc = check_hip(hipMemset(sc.colsum, 0, sizeof(ColSums)), "hipMemset");
        if (!rc && hd == 0 && net->heads == 2) {
            rc = check_hip(hipMalloc(reinterpret_cast<void **>(&net->colsum3), sizeof(ColSums)), "hipMalloc");
            if (!rc) rc = check_hip(hipMemset(net->colsum3, 0, sizeof(ColSums)), "hipMemset");
            if (!rc) rc = check_hip(hipStreamSynchronize(nullptr), "hipStreamSynchronize");  // (the heads' streams are non-blocking: see alloc_planes)
        }
        if (!rc) rc = check_hip(hipStreamSynchronize(nullptr), "hipStreamSynchronize");  // (see alloc_planes)
        if (!rc) rc = check_hip(hipStreamCreateWithFlags(&sc.side, hipStreamNonBlocking), "hipStreamCreate");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&sc.ev_fork, event_flags()), "hipEventCreate");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&sc.ev_join, event_flags()), "hipEventCreate");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&sc.ev_entry, event_flags()), "hipEventCreate");
    }
    if (!rc && net->heads == 2) {
        rc = check_hip(hipStreamCreateWithFlags(&net->head1, hipStreamNonBlocking), "hipStreamCreate");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&net->ev_head_fork, event_flags()), "hipEventCreate");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&net->ev_head_join, event_flags()), "hipEventCreate");
    }
    if (!rc) rc = alloc_planes(&net->YY, np, net->heads * os);
    if (!rc) rc = alloc_planes(&net->Y3, np, os);
    if (!rc && plan.head_layers) rc = alloc_planes(&net->PA, np, os);
    if (!rc && plan.head_layers) rc = alloc_planes(&net->PB, np, os);
    if (!rc) rc = check_hip(hipStreamCreateWithFlags(&net->cap, hipStreamNonBlocking), "hipStreamCreate");
    {
        const char *g = getenv("OJF_NET_GRAPH");  // opt-in: see the note at ojf_net::cap
        net->use_graph = g && g[0] == '1';
    }
    if (rc) {
        const std::string keep = ojf_last_error();
        ojf_net_destroy(net);
        set_error(keep);
        return rc;
    }
    *out = net;
    return 0;
}

namespace ojf {
int net_input_slot(::ojf_net *net, NetInputSlot *slot)
{
    if (!net || !slot || net->sem || net->heads != 1) return 1;
    slot->x0 = net->X[0]; slot->cs4 = net->cs / 4; slot->P = net->P; slot->h = net->h; slot->w = net->w;
    slot->ovf = net->arith == OJF_ARITH_F16X3 ? overflow_flag() : nullptr;
    slot->split = net->plan.dense == DENSE_CHAIN ? 1 : 0;
    return 0;
}
}  // namespace ojf

OJF_API int ojf_net_prepare_input(ojf_net *net, const float *values, const float *weights, int rows_stride,
                                  int in_layout, const float *depth, const uint8_t *sem_ids, int n_classes, ojf_stream_t stream)
{
    using namespace ojf;
    if (!net || !values || !weights || !depth) return fail("ojf_net_prepare_input: null pointer argument");
    if (in_layout != 0 && in_layout != 1) return fail("ojf_net_prepare_input: in_layout must be 0 or 1");
    if (in_layout == 0 && rows_stride < net->P) return fail("ojf_net_prepare_input: rows_stride < n_points");
    if (in_layout == 1 && rows_stride < net->npix) return fail("ojf_net_prepare_input: plane stride < h*w");
    if (net->sem && (!sem_ids || n_classes <= 0))
        return fail("ojf_net_prepare_input: this net uses semantics: sem_ids and n_classes are required");
    PrepArgs a;
    a.values = values; a.weights = weights; a.depth = depth;
    a.sem = net->sem ? sem_ids : nullptr;
    a.x0 = planes(net->X[0]);
    a.x1 = net->heads == 2 ? planes(net->X[1]) : nullptr;
    a.rows_stride = rows_stride; a.in_layout = in_layout; a.npix = net->npix; a.P = net->P; a.cs4 = net->cs / 4;
    a.n_classes = n_classes;
    a.v2_sem = (net->version == 2 && net->sem) ? 1 : 0;
    a.ovf = net->arith == OJF_ARITH_F16X3 ? overflow_flag() : nullptr;
    a.split = net->plan.dense == DENSE_CHAIN ? 1 : 0;
    hipLaunchKernelGGL(prepare_input_kernel, dim3((a.npix + 255) / 256), dim3(256), 0, as_stream(stream), a);
    return check_hip(hipGetLastError(), "prepare_input_kernel launch");
}

namespace ojf {

// Two HIP streams only run concurrently when the runtime maps them to different hardware queues (a small round-robin
// pool): a second-head stream that aliases the launch stream's queue silently serialises the two heads (measured:
// net stage 0.60 -> 0.70 ms for the two-head net when the library is used by the third engine of a process).  The
// pairing is therefore TESTED once per (net, launch stream): two 150 us spin kernels, one per stream, take ~150 us
// when the streams overlap and ~300 us when they do not; up to 8 fresh streams are tried per role.
__global__ void spin_kernel(long long cycles)
{
    const long long t0 = (long long)__builtin_amdgcn_s_memtime();
    while ((long long)__builtin_amdgcn_s_memtime() - t0 < cycles) __builtin_amdgcn_s_sleep(32);
}

static double spin_pair_us(hipStream_t a, hipStream_t b, long long cycles)
{
    (void)hipStreamSynchronize(a);
    (void)hipStreamSynchronize(b);
    const auto t0 = std::chrono::steady_clock::now();
    // a's spin is followed by a kernel that DEPENDS on it: two streams that share a hardware queue run independent kernels
    // side by side, but the barrier packet in front of a dependent one holds back every later packet of that queue, the
    // other stream's included (round 5: a look-ahead stream that passed the two-spins test shared the queue of the
    // second head's stream and ran 20 % slower than one that did not)
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, cycles);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a, 1LL);
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b, cycles);
    (void)hipStreamSynchronize(a);
    (void)hipStreamSynchronize(b);
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

// makes `s` a stream that overlaps with every stream of `others` (replaces it by fresh ones until the test passes)
static void pair_stream(hipStream_t &s, const hipStream_t *others, int n, double alone, long long cycles)
{
    std::vector<hipStream_t> rejected;
    for (int attempt = 0; attempt < 8; ++attempt) {
        double worst = 0.0;
        for (int k = 0; k < n; ++k) {
            const double both = spin_pair_us(others[k], s, cycles);
            worst = both > worst ? both : worst;
        }
        if (worst < 1.5 * alone) break;  // overlaps with all of them
        // the replacement is created while the rejected streams still exist: a stream created right after a destroy
        // gets the freed queue slot again
        hipStream_t fresh = nullptr;
        if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) break;
        rejected.push_back(s);
        s = fresh;
    }
    for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
}

}  // namespace ojf

OJF_API int ojf_streams_overlap(ojf_stream_t a, ojf_stream_t b)
{
    using namespace ojf;
    hipStream_t sa = as_stream(a), sb = as_stream(b);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(sa, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return fail("ojf_streams_overlap: stream a is capturing");
    if (hipStreamIsCapturing(sb, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return fail("ojf_streams_overlap: stream b is capturing");
    const long long cycles = 300000;  // ~130 us
    (void)spin_pair_us(sa, sb, 1000);  // (the first launch of the kernel in a process loads its code object)
    double alone = 1e30, both = 1e30;
    for (int rep = 0; rep < 2; ++rep) {
        const double t1 = spin_pair_us(sa, sa, cycles) * 0.5;  // two spins back to back on one stream
        const double t2 = spin_pair_us(sa, sb, cycles);
        alone = t1 < alone ? t1 : alone;
        both = t2 < both ? t2 : both;
    }
    if (hipGetLastError() != hipSuccess) return fail("ojf_streams_overlap: spin kernel launch failed");
    return both < 1.5 * alone ? 1 : 0;
}

namespace ojf {

static void pair_head_stream(ojf_net *net, hipStream_t st)
{
    if (net->heads != 2 || (net->head_paired && net->head_paired_with == st) || !net->head1) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return;  // not inside a capture
    net->head_paired_with = st;
    net->head_paired = true;
    const long long cycles = 300000;  // ~130 us
    (void)spin_pair_us(st, st, 1000);  // (the first launch of the kernel in a process loads its code object: not in the yardstick)
    const double alone = spin_pair_us(st, st, cycles) * 0.5;  // two spins back to back on one stream
    pair_stream(net->head1, &st, 1, alone, cycles);
    // the side streams of the general VortexPooling flow (global-average branch, branch 0): each must overlap with the
    // stream of ITS head (only three queues ran concurrently in every test, so four-way distinctness is not asked for)
    if (net->sc[1].side) pair_stream(net->sc[1].side, &net->head1, 1, alone, cycles);
    if (net->sc[0].side) pair_stream(net->sc[0].side, &st, 1, alone, cycles);
}

// every launch of one forward pass, in the plan's order, on `st` (+ the second head's stream and the side streams, forked and
// joined with events).  Per call: the stream, est / est_stride, and whether the second head's stream is distinct from `st`.
static int forward_launches(ojf_net *net, float *est, int est_stride, hipStream_t st)
{
    const int o4 = net->os / 4;
    // prediction head: 1x1 chain; BN-folded LeakyReLU stages, the last layer is Tanh * output_scale
    ChainArgs ca;
    ca.in = planes(net->Y3); ca.w = planes(net->chain_w); ca.bias = net->chain_b;
    ca.out_rows = est; ca.in_g0 = 0; ca.c4_in = o4; ca.npix = net->npix;
    ca.rows_stride = est_stride; ca.rows_n = net->P; ca.scale = net->scale;
    ca.ovf = net->arith == OJF_ARITH_F16X3 ? overflow_flag() : nullptr;
    const ForwardPlan &plan = net->plan;
    const bool two = plan.n_steps == 3;
    if (two) pair_head_stream(net, st);
    hipStream_t s1 = two ? net->head1 : st;
    if (two && s1 != st) {  // the semantic head runs beside the geometric one
        OJF_HIP(hipEventRecord(net->ev_head_fork, st));
        OJF_HIP(hipStreamWaitEvent(s1, net->ev_head_fork, 0));
    }
    for (int i = 0; i < plan.n_steps; ++i) {
        const VortexStep &s = plan.step[i];
        hipStream_t ss = s.vortex == 1 ? s1 : st;
        if (s.vortex < 2) {  // a head: its dense Blocks first
            if (run_dense(net, s.vortex, ss)) return -2;
        } else if (two && s1 != st) {  // the last VortexPooling reads both heads' results
            OJF_HIP(hipEventRecord(net->ev_head_join, s1));
            OJF_HIP(hipStreamWaitEvent(st, net->ev_head_join, 0));
        }
        if (run_vortex(net, s, ss, ca)) return -2;
    }
    if (!plan.head_layers) return 0;
    const float *pin = net->Y3;
    const int np = (int)net->pred.size();
    float *pp[2] = {net->PA, net->PB};
    for (int i = 0; i < np; ++i) {
        const PackedConv &pc = net->pred[i];
        const bool last = (i == np - 1);
        if (last) {  // exactly n_points channels into the caller's row-major est
            if (launch_conv(pc, pin, 0, nullptr, 0, nullptr, OJF_ACT_TANH, pc.n_ot * 16, net->scale, net->h, net->w, st,
                            est, est_stride, net->P)) return -2;
        } else {
            if (launch_conv(pc, pin, 0, pp[i & 1], 0, nullptr, OJF_ACT_LEAKY, pc.n_ot * 16, 1.0f, net->h, net->w, st))
                return -2;
            pin = pp[i & 1];
        }
    }
    return 0;
}

static void drop_graph(ojf_net *net)
{
    if (net->gexec) (void)hipGraphExecDestroy(net->gexec);
    if (net->graph) (void)hipGraphDestroy(net->graph);
    net->gexec = nullptr;
    net->graph = nullptr;
}

// Records the ~30 launches of a forward pass (both streams) once per (est, est_stride) into a hipGraph.
// The capture runs on the net's own stream: the caller's stream may be the legacy default stream, which
// cannot be captured but can launch a graph.  A failed capture disables graphs for this net (plain launches).
static void capture_graph(ojf_net *net, float *est, int est_stride)
{
    drop_graph(net);
    net->g_est = est;
    net->g_stride = est_stride;
    // (no allocation happens while capturing: every buffer of the plan exists since ojf_net_create)
    if (hipStreamBeginCapture(net->cap, hipStreamCaptureModeThreadLocal) != hipSuccess) { net->use_graph = false; return; }
    const int rc = forward_launches(net, est, est_stride, net->cap);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(net->cap, &g);
    if (rc || e != hipSuccess || !g || hipGraphInstantiate(&net->gexec, g, nullptr, nullptr, 0) != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        net->gexec = nullptr;
        net->use_graph = false;
        (void)hipGetLastError();
        return;
    }
    net->graph = g;
}

}  // namespace ojf

OJF_API int ojf_net_forward(ojf_net *net, float *est, int est_stride, ojf_stream_t stream)
{
    using namespace ojf;
    if (!net || !est) return fail("ojf_net_forward: null pointer argument");
    if (est_stride < net->P) return fail("ojf_net_forward: est_stride < n_points");
    hipStream_t st = as_stream(stream);
    if (net->arith == OJF_ARITH_F16X3)
        if (const int rc = guard_refusal()) return rc;
    if (net->use_graph) {
        if (!net->gexec || net->g_est != est || net->g_stride != est_stride) capture_graph(net, est, est_stride);
        if (net->gexec) return check_hip(hipGraphLaunch(net->gexec, st), "hipGraphLaunch (net forward)");
    }
    const int before = g_launches;
    const int rc = forward_launches(net, est, est_stride, st);
    net->last_launches = g_launches - before;
    return rc;
}

OJF_API int64_t ojf_net_macs_per_pixel(const ojf_net *net) { return net ? net->macs_per_pixel : -1; }

OJF_API int ojf_net_launch_count(const ojf_net *net) { return net ? net->last_launches : -1; }

OJF_API int ojf_net_side_streams(ojf_net *net, ojf_stream_t stream, ojf_stream_t out[3])
{
    using namespace ojf;
    if (!net || !out) return fail("ojf_net_side_streams: null pointer argument");
    pair_head_stream(net, as_stream(stream));  // (what the first forward pass on `stream` would do; a no-op for one head / inside a capture)
    out[0] = net->heads == 2 ? reinterpret_cast<ojf_stream_t>(net->head1) : nullptr;
    out[1] = reinterpret_cast<ojf_stream_t>(net->sc[0].side);
    out[2] = net->heads == 2 ? reinterpret_cast<ojf_stream_t>(net->sc[1].side) : nullptr;
    return (out[0] != nullptr) + (out[1] != nullptr) + (out[2] != nullptr);
}

OJF_API int ojf_net_profile(ojf_net *net, float *est, int est_stride, ojf_stream_t stream, char *names, int names_cap,
                            float *micros, int max_entries)
{
    using namespace ojf;
    if (!net || !est || !names || !micros || names_cap < 1 || max_entries < 1) return fail("ojf_net_profile: bad argument");
    hipStream_t st = as_stream(stream);
    hipEvent_t e0 = nullptr;
    OJF_HIP(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));
    g_marks.clear();
    g_profile = true;
    (void)hipEventRecord(e0, st);
    const int rc = forward_launches(net, est, est_stride, st);
    g_profile = false;
    int n = 0;
    size_t used = 0;
    names[0] = 0;
    if (!rc && hipStreamSynchronize(st) == hipSuccess) {
        for (size_t i = 0; i < g_marks.size() && n < max_entries; ++i) {
            // previous mark on the same stream (the start mark for the first launch of the caller's stream)
            hipEvent_t prev = nullptr;
            for (size_t j = i; j-- > 0;)
                if (g_marks[j].st == g_marks[i].st) { prev = g_marks[j].ev; break; }
            if (!prev && g_marks[i].st == st) prev = e0;
            float ms = 0.0f;
            (void)hipEventSynchronize(g_marks[i].ev);
            if (!prev || hipEventElapsedTime(&ms, prev, g_marks[i].ev) != hipSuccess) ms = -1e-3f;  // first launch of a side stream
            const size_t len = strlen(g_marks[i].name);
            if (used + len + 2 > (size_t)names_cap) break;
            memcpy(names + used, g_marks[i].name, len);
            names[used + len] = '\n';
            used += len + 1;
            names[used] = 0;
            micros[n++] = ms * 1e3f;
        }
    }
    for (auto &m : g_marks) (void)hipEventDestroy(m.ev);
    g_marks.clear();
    (void)hipEventDestroy(e0);
    return rc ? rc : n;
}

OJF_API int ojf_net_plan(int version, int n_points, int growth, int use_semantics, int h, int w, int arithmetic, char *names,
                         int names_cap)
{
    using namespace ojf;
    if (!names || names_cap < 1) return refuse("ojf_net_plan", "bad argument");
    if (arithmetic != OJF_ARITH_F32 && arithmetic != OJF_ARITH_F16X3) return refuse("ojf_net_plan", "unknown arithmetic (OJF_ARITH_F32 or OJF_ARITH_F16X3)");
    NetShape shape;
    ForwardPlan plan;
    if (const char *why = net_shape(shape, version, n_points, growth, use_semantics, h, w, arithmetic)) return refuse("ojf_net_plan", why);
    if (const char *why = plan_forward(shape, &plan)) return refuse("ojf_net_plan", why);
    const std::vector<Launch> launches = plan_launches(shape, plan);
    size_t used = 0;
    names[0] = 0;
    for (Launch l : launches) {
        const size_t len = strlen(kLaunchNames[l]);
        if (used + len + 2 > (size_t)names_cap) return refuse("ojf_net_plan", "names buffer too small");
        memcpy(names + used, kLaunchNames[l], len);
        names[used + len] = '\n';
        used += len + 1;
        names[used] = 0;
    }
    return (int)launches.size();
}

OJF_API int ojf_net_set_arithmetic(int arithmetic)
{
    if (arithmetic != OJF_ARITH_F32 && arithmetic != OJF_ARITH_F16X3)
        return ojf::fail("ojf_net_set_arithmetic: unknown arithmetic (OJF_ARITH_F32 or OJF_ARITH_F16X3)");
    ojf::g_default_arith = arithmetic;
    return 0;
}

OJF_API int ojf_net_get_arithmetic(const ojf_net *net) { return net ? net->arith : ojf::g_default_arith; }

OJF_API int ojf_conv2d(const float *in, int in_stride, int in_off, float *out, int out_stride, int out_off,
                       const ojf_conv_layer *layer, int act, int h, int w, ojf_stream_t stream)
{
    using namespace ojf;
    if (!in || !out || !layer || !layer->weight_host || !layer->bias_host) return fail("ojf_conv2d: null pointer argument");
    if ((layer->ksize != 1 && layer->ksize != 3) || layer->dilation < 1) return fail("ojf_conv2d: 1x1 or 3x3 kernels only");
    const int cin_phys = round_up(layer->c_in, 4), cout_phys = round_up(layer->c_out, 4);
    if (in_off + layer->c_in > in_stride || out_off + cout_phys > out_stride)
        return fail("ojf_conv2d: channel window exceeds the row stride");
    hipStream_t st = as_stream(stream);
    const int npix = h * w;
    ConvBuilder b(cin_phys, cout_phys, layer->ksize, layer->dilation);
    b.add(*layer, 0, layer->c_in, slot_map(layer->c_in, layer->c_in, cin_phys), 0, true);
    PackedConv pc;
    if (finish(b, pc, g_default_arith)) return -2;
    float *pin = nullptr, *pout = nullptr;
    int rc = alloc_planes(&pin, npix, cin_phys);
    if (!rc) rc = alloc_planes(&pout, npix, cout_phys);
    if (!rc) {
        hipLaunchKernelGGL(rows_to_planes_kernel, dim3((npix * (cin_phys / 4) + 255) / 256), dim3(256), 0, st, in, in_stride,
                           in_off, layer->c_in, planes(pin), cin_phys / 4, npix);
        rc = launch_conv(pc, pin, 0, pout, 0, nullptr, act, cout_phys, 1.0f, h, w, st);
    }
    if (!rc) {
        hipLaunchKernelGGL(planes_to_rows_kernel, dim3((npix * (cout_phys / 4) + 255) / 256), dim3(256), 0, st,
                           planes(pout), cout_phys / 4, npix, out, out_stride, out_off);
        rc = check_hip(hipStreamSynchronize(st), "ojf_conv2d sync");  // test-only API: packs per call
        if (!rc && guard_take(nullptr, true)) rc = guard_fail(1);
    }
    free_planes(pin);
    free_planes(pout);
    release(pc);
    return rc;
}

OJF_API int ojf_pool_pyramid(const float *z, const float *z2, float *q1, float *q2, float *q3, float *q0, const float *bias1,
                             const float *bias2, const float *bias3, const float *bias0, int h, int w, int c4, int split_out,
                             void *colsums, const float *wg_t, const float *bg, const float *wfg_t, const float *bf, int cphys,
                             int c_out, float *bias_out, int bias_len, ojf_stream_t stream)
{
    using namespace ojf;
    if (!z || !q1 || !q2 || !q3 || !bias1 || !bias2 || !bias3) return fail("ojf_pool_pyramid: null pointer argument");
    if (z2 && (!q0 || !bias0)) return fail("ojf_pool_pyramid: z2 needs q0 and bias0");
    if (h < 1 || w < 1 || c4 < 1 || c4 > 64 || (int64_t)h * w > (1 << 24)) return fail("ojf_pool_pyramid: bad frame size or group count");
    PyramidArgs pa;
    pa.z = planes(z); pa.z2 = z2 ? planes(z2) : nullptr;
    pa.q[0] = planes(q1); pa.q[1] = planes(q2); pa.q[2] = planes(q3); pa.q0 = z2 ? planes(q0) : nullptr;
    pa.bias[0] = bias1; pa.bias[1] = bias2; pa.bias[2] = bias3; pa.bias0 = z2 ? bias0 : nullptr;
    pa.h = h; pa.w = w; pa.c4 = c4;
    pa.split_out = split_out ? 1 : 0;
    pa.fold_gave = colsums ? 1 : 0;
    pa.gave = GaveArgs{};
    if (colsums) {
        if (!wg_t || !bg || !wfg_t || !bf || !bias_out) return fail("ojf_pool_pyramid: null pointer argument (fold)");
        if (cphys < 1 || cphys > kColMax || c_out < 1 || c_out > 256 || bias_len < 0 || bias_len > 256)
            return fail("ojf_pool_pyramid: fold sizes beyond one block (256)");
        GaveArgs &ga = pa.gave;
        ga.partial = nullptr; ga.fixed = static_cast<ColSums *>(colsums); ga.nparts = 0; ga.pstride = 0; ga.cphys = cphys; ga.npix = h * w;
        ga.WgT = wg_t; ga.bg = bg; ga.WfgT = wfg_t; ga.bf = bf; ga.c_out = c_out;
        ga.bias_out = bias_out; ga.bias_len = bias_len;
    }
    launch_pyramid(pa, as_stream(stream));
    return check_hip(hipGetLastError(), "ojf_pool_pyramid launch");
}

OJF_API int ojf_entry_gemm(const float *weight, const float *bias, int c_in_phys, int cs, const float *in, int in_split, int c4_in,
                           int npix, float *out, int og_store, int split_groups, int act_n, void *colsums, int form,
                           int max_blocks, ojf_stream_t stream)
{
    using namespace ojf;
    if (!weight || !bias || !in || !out || !colsums) return fail("ojf_entry_gemm: null pointer argument");
    if (c_in_phys < 4 || c_in_phys > 128 || c_in_phys % 4 || cs < 4 || cs > 20 || cs % 4)
        return fail("ojf_entry_gemm: the 8-tile form takes up to 128 input channels and 4 slots of up to 20, both multiples of 4");
    if (c4_in < 1 || c4_in * 4 > c_in_phys || npix < 1 || npix > (1 << 24) || og_store < 0 || og_store > cs || split_groups < 0 || split_groups > cs || act_n < 0 ||
        (form != 0 && form != 1) || max_blocks < 0)
        return fail("ojf_entry_gemm: bad sizes");
    hipStream_t st = as_stream(stream);
    auto we = [&](int oc, int k) { return oc < 4 * cs && k < c_in_phys ? weight[(size_t)oc * c_in_phys + k] : 0.0f; };
    const std::vector<float> re = chain_row_scales(OJF_ARITH_F16X3, 5, c_in_phys, we);
    std::vector<float> ew, eb;
    pack_chain_layer(ew, OJF_ARITH_F16X3, 5, 8, re, we);
    append_chain_bias(eb, OJF_ARITH_F16X3, 5, 4 * cs, bias, re);
    float *dw = nullptr, *db = nullptr;
    int rc = upload(ew, &dw);
    if (!rc) rc = upload(eb, &db);
    if (!rc) {
        ChainArgs ea;
        ea.in = planes(in); ea.w = planes(dw); ea.bias = db; ea.out_rows = nullptr;
        ea.in_g0 = 0; ea.c4_in = c4_in; ea.npix = npix; ea.rows_stride = 0; ea.rows_n = 0; ea.scale = 1.0f;
        ea.ovf = overflow_flag();
        ea.out_planes = planes(out); ea.out_g0 = 0; ea.og_store = og_store; ea.act_n = act_n; ea.colsum = static_cast<ColSums *>(colsums);
        ea.split_groups = split_groups;
        ea.in_split = in_split ? 1 : 0;
        const int strips = ((npix + 15) / 16 + kChainWaves - 1) / kChainWaves;
        if (form == 1) launch_entry_persistent(ea, strips, max_blocks, st);
        else hipLaunchKernelGGL((entry1x1_kernel<OJF_ARITH_F16X3, 1, 8, 5>), dim3(strips), dim3(kChainThreads), 0, st, ea);
        rc = check_hip(hipGetLastError(), "ojf_entry_gemm launch");
        if (!rc) rc = check_hip(hipStreamSynchronize(st), "ojf_entry_gemm sync");  // test-only API: packs per call
    }
    if (dw) (void)hipFree(dw);
    if (db) (void)hipFree(db);
    return rc;
}

OJF_API int ojf_vortex_tail(int kind, const float *w1, const float *b1, const float *wf, const float *bf, int c, int c_out,
                            const float *next_w, const float *next_b, const int *next_dims, const float *v, int c4, int npix,
                            float *out, int og_store, int split_groups, int act_n, void *colsums, int rows_stride, int rows_n,
                            float scale, int form, ojf_stream_t stream)
{
    using namespace ojf;
    constexpr int NV = 2, NO = 8, A = OJF_ARITH_F16X3;
    static const int head_tiles[12] = {8, 6, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1};  // head_run's growth-19 topology
    if (!w1 || !b1 || !wf || !bf || !next_w || !next_b || !next_dims || !v || !out) return fail("ojf_vortex_tail: null pointer argument");
    if (kind != kTailEntry && kind != 19) return fail("ojf_vortex_tail: kind must be 1 (+ entry GEMM) or 19 (+ prediction head)");
    if (kind == kTailEntry && !colsums) return fail("ojf_vortex_tail: null pointer argument (colsums)");
    if (c < 1 || c > 16 * NV || c_out < 1 || (c_out + 15) / 16 != NO || c4 < 1 || c4 > 4 * NV || 4 * c4 < c)
        return fail("ojf_vortex_tail: the fused tail takes up to 32 branch channels in c4 groups and 113..128 output channels");
    if (npix < 1 || npix > (1 << 24) || (form != 0 && form != 1)) return fail("ojf_vortex_tail: bad sizes");
    if (kind == kTailEntry) {
        const int cs = next_dims[0];
        if (cs < 4 || cs > 20 || cs % 4 || og_store < 0 || og_store > cs || split_groups < 0 || split_groups > cs || act_n < 0)
            return fail("ojf_vortex_tail: bad entry layer sizes");
    } else {
        if (next_dims[0] != c_out) return fail("ojf_vortex_tail: the head's first layer reads the tail's channels");
        for (int l = 0; l < 12; ++l)
            if (next_dims[l] < 1 || (round_up(next_dims[l], 4) + 15) / 16 != head_tiles[l])
                return fail("ojf_vortex_tail: the head's channel counts do not fit the 8-6-6-5-5-4-4-3-3-2-2-1 tile chain");
        if (rows_n < 1 || rows_n > next_dims[11] || rows_stride < rows_n) return fail("ojf_vortex_tail: bad row sizes");
    }
    hipStream_t st = as_stream(stream);
    // packed as build_vortex packs the net's: [W1_b | Wf_b] fragments per branch, one common row scale for the four column blocks
    std::vector<float> tw, tb, nw, nb, bfin((size_t)NO * 16, 0.0f);
    const std::vector<float> rf = chain_row_scales(A, NO, 4 * c_out, [&](int oc, int k) { return oc < c_out ? wf[(size_t)oc * 4 * c_out + k] : 0.0f; });
    for (int br = 0; br < 4; ++br) {
        auto wb = [&](int oc, int k) { return oc < c_out && k < c ? w1[((size_t)br * c_out + oc) * c + k] : 0.0f; };
        const std::vector<float> r1 = chain_row_scales(A, NO, c, wb);
        pack_chain_layer(tw, A, NO, NV, r1, wb);
        pack_chain_layer(tw, A, NO, NO, rf, [&](int oc, int k) { return oc < c_out && k < c_out ? wf[(size_t)oc * 4 * c_out + (size_t)c_out * br + k] : 0.0f; });
        append_chain_bias(tb, A, NO, c_out, b1 + (size_t)br * c_out, r1);
    }
    std::vector<float> rfi(rf.size());
    for (size_t i = 0; i < rf.size(); ++i) rfi[i] = 1.0f / rf[i];
    for (int o = 0; o < c_out; ++o) bfin[o] = bf[o];
    if (kind == kTailEntry) {
        const int cs = next_dims[0];
        auto we = [&](int oc, int k) { return oc < 4 * cs && k < c_out ? next_w[(size_t)oc * c_out + k] : 0.0f; };
        const std::vector<float> re = chain_row_scales(A, 5, c_out, we);
        pack_chain_layer(nw, A, 5, 8, re, we);
        append_chain_bias(nb, A, 5, 4 * cs, next_b, re);
    } else {
        const float *wl0 = next_w, *bl0 = next_b;
        for (int l = 0; l < 11; ++l) {
            const int ci = next_dims[l], co = next_dims[l + 1];
            auto wl = [&](int oc, int k) { return oc < co && k < ci ? wl0[(size_t)oc * ci + k] : 0.0f; };
            const std::vector<float> rs = chain_row_scales(A, head_tiles[l + 1], ci, wl);
            pack_chain_layer(nw, A, head_tiles[l + 1], head_tiles[l], rs, wl);
            append_chain_bias(nb, A, head_tiles[l + 1], co, bl0, rs);
            wl0 += (size_t)co * ci;
            bl0 += co;
        }
    }
    float *dtw = nullptr, *dtb = nullptr, *dnw = nullptr, *dnb = nullptr, *dbf = nullptr, *dri = nullptr;
    int rc = upload(tw, &dtw);
    if (!rc) rc = upload(tb, &dtb);
    if (!rc) rc = upload(nw, &dnw);
    if (!rc) rc = upload(nb, &dnb);
    if (!rc) rc = upload(bfin, &dbf);
    if (!rc) rc = upload(rfi, &dri);
    if (!rc) {
        TailArgs ta;
        for (int br = 0; br < 4; ++br) ta.v[br] = planes(v) + (size_t)br * c4 * npix;
        ta.w = planes(dtw); ta.b1 = dtb; ta.bias_final = dbf; ta.rinv_final = dri;
        ta.out = nullptr; ta.c4 = c4; ta.out_g0 = 0; ta.og_store = 0; ta.npix = npix;
        ta.ovf = overflow_flag();
        ta.chain_w = nullptr; ta.chain_b = nullptr; ta.out_rows = nullptr; ta.rows_stride = 0; ta.rows_n = 0; ta.scale = 1.0f;
        ta.entry_w = nullptr; ta.entry_b = nullptr; ta.entry_out = nullptr; ta.entry_og = 0; ta.entry_act_n = 0; ta.colsum = nullptr; ta.entry_split = 0;
        const dim3 grid(((npix + 15) / 16 + kChainWaves - 1) / kChainWaves), block(kChainThreads);
        if (kind == kTailEntry) {
            ta.entry_w = planes(dnw); ta.entry_b = dnb; ta.entry_out = planes(out);
            ta.entry_og = og_store; ta.entry_act_n = act_n; ta.colsum = static_cast<ColSums *>(colsums); ta.entry_split = split_groups;
            if (form == 1) hipLaunchKernelGGL((vortex_tail_kernel<A, 1, NV, NO, kTailEntry>), grid, block, 0, st, ta);
            else hipLaunchKernelGGL((vortex_tail_kernel<A, 1, NV, NO, kTailEntry, kTailAtBranch>), grid, block, 0, st, ta);
        } else {
            ta.chain_w = planes(dnw); ta.chain_b = dnb; ta.out_rows = out; ta.rows_stride = rows_stride; ta.rows_n = rows_n; ta.scale = scale;
            if (form == 1) hipLaunchKernelGGL((vortex_tail_kernel<A, 1, NV, NO, 19>), grid, block, 0, st, ta);
            else hipLaunchKernelGGL((vortex_tail_kernel<A, 1, NV, NO, 19, kTailAtBranch>), grid, block, 0, st, ta);
        }
        rc = check_hip(hipGetLastError(), "ojf_vortex_tail launch");
        if (!rc) rc = check_hip(hipStreamSynchronize(st), "ojf_vortex_tail sync");  // test-only API: packs per call
    }
    for (float *d : {dtw, dtb, dnw, dnb, dbf, dri})
        if (d) (void)hipFree(d);
    return rc;
}

#ifdef OJF_POOL_STAMPS
extern "C" __attribute__((visibility("default"))) int ojf_debug_pool_stamps(void *host_dst, size_t bytes)
{
    return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(ojf::g_pool_stamps), bytes < sizeof(ojf::g_pool_stamps) ? bytes : sizeof(ojf::g_pool_stamps));
}
#endif

#ifdef OJF_TAIL_STAMPS
extern "C" __attribute__((visibility("default"))) int ojf_debug_tail_stamps(void *host_dst, size_t bytes)
{
    return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(ojf::g_tail_stamps), bytes < sizeof(ojf::g_tail_stamps) ? bytes : sizeof(ojf::g_tail_stamps));
}
extern "C" __attribute__((visibility("default"))) int ojf_debug_tail_form(int form)  // 0 requests at each branch's head, 1 one branch ahead (the product)
{
    if (form < 0 || form > 1) return -1;
    ojf::g_tail_stamp_form = form;
    return 0;
}
#endif

#ifdef OJF_ENTRY_STAMPS
extern "C" __attribute__((visibility("default"))) int ojf_debug_entry_stamps(void *host_dst, size_t bytes)
{
    return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(ojf::g_entry_stamps), bytes < sizeof(ojf::g_entry_stamps) ? bytes : sizeof(ojf::g_entry_stamps));
}
#endif
