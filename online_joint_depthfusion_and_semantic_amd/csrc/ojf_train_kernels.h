// Device kernels of the fusion net's TRAINING path and their argument structs: first those of the layer units (packing,
// BatchNorm statistics, normalise + activate, weight gradient, average pool), then those of the whole-net executor (input /
// output layout, pool pyramid, global-average branch, fuse-output and loss glue, split-fp16 weight packing).  The design
// and the host side are in ojf_train.hip; the convolutions themselves are ojf_net.hip's, reached through launch_conv_args.
#pragma once
#include "ojf_net_conv.h"

namespace ojf {

constexpr int kTrainSlabs = 64;  // pixel slabs of the per-channel reductions (partial sums added in slab order)

// ---- weight packing on the device ----------------------------------------------------------------------------------
// Packed element (row r, K group G = tap * c4 + cg, component j) <- weight(oc, ic, tap'):
//   forward:     oc = r,            ic = unslot(4 cg + j),  tap' = tap
//   transposed:  ic = unslot(r),    oc = 4 cg + j,          tap' = taps - 1 - tap   (backward-data)
// unslot: physical channel of a concatenation of `group`-wide tensors stored in `slot`-wide slots -> logical channel.
struct PackArgs {
    const float *w;     // [OC][IC][taps]
    const float *bias;  // [OC] or NULL
    float *wp;          // [n_ot][nsteps + kPadSteps][64][4]
    float *bp;          // [n_ot * 16] (forward form only; NULL otherwise)
    int OC, IC, taps, group, slot, c4, nsteps, n_ot, transposed;
    // stacked layers (the four branch-entry 1x1 of a VortexPooling as ONE convolution): this weight tensor owns output
    // channels [oc_base, oc_base + OC) of the stack; with `partial` only its elements are written (the buffer starts zeroed)
    int oc_base, partial;
    // a convolution that reads only input channels [ic_base, ic_base + IC) of a weight tensor with ic_total input channels
    int ic_base, ic_total;
};

__device__ __forceinline__ int train_unslot(int x, int group, int slot, int n_logical)
{
    const int s = x / slot, in = x - s * slot;
    const int l = s * group + in;
    return (in < group && l < n_logical) ? l : -1;
}

__global__ __launch_bounds__(256) void train_pack_kernel(const PackArgs a)
{
    const int nsp = a.nsteps + kPadSteps;
    const long total = (long)a.n_ot * nsp * 256;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)a.n_ot * 16 && a.bp) {
        const long ob = i - a.oc_base;
        const bool mine = ob >= 0 && ob < a.OC;
        if (mine || !a.partial) a.bp[i] = (a.bias && mine) ? a.bias[ob] : 0.0f;
    }
    if (i >= total) return;
    const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
    const long rest = i >> 8;
    const int S = (int)(rest % nsp), ot = (int)(rest / nsp);
    const int r = ot * 16 + (lane & 15), G = 4 * S + (lane >> 4);
    float v = 0.0f;
    bool mine = false;
    if (S < a.nsteps && G < a.taps * a.c4) {
        const int tap = G / a.c4, ch = 4 * (G - tap * a.c4) + j;
        int oc, ic, t;
        if (!a.transposed) { oc = r - a.oc_base; ic = train_unslot(ch, a.group, a.slot, a.IC); t = tap; }
        else { ic = train_unslot(r, a.group, a.slot, a.IC); oc = ch - a.oc_base; t = a.taps - 1 - tap; }
        mine = oc >= 0 && oc < a.OC;
        if (mine && ic >= 0) v = a.w[((size_t)oc * a.ic_total + a.ic_base + ic) * a.taps + t];
    }
    if (mine || !a.partial) a.wp[i] = v;
}

// ---- BatchNorm statistics ------------------------------------------------------------------------------------------
// block (slab, channel group): fp64 sums of y and y^2 over the slab's pixels of the group's four channels
__device__ __forceinline__ void train_stats_partial_body(const f32x4 *y, int g0, int npix, double *partial /* [slabs][c4][8] */)
{
    __shared__ double red[4][8];
    const int cg = blockIdx.y, c4 = gridDim.y;
    const int per = (npix + kTrainSlabs - 1) / kTrainSlabs;
    const int p0 = blockIdx.x * per, p1 = min(npix, p0 + per);
    const f32x4 *plane = y + (size_t)(g0 + cg) * npix;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // four loads in flight per lane (the kernels of this file are latency-, not bandwidth-bound); the sums run in the
    // same order as a plain loop
    int p = p0 + threadIdx.x;
    for (; p + 768 < p1; p += 1024) {
        const f32x4 v4[4] = {plane[p], plane[p + 256], plane[p + 512], plane[p + 768]};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) { s[j] += (double)v4[u][j]; s[4 + j] += (double)v4[u][j] * (double)v4[u][j]; }
    }
    for (; p < p1; p += 256) {
        const f32x4 v = plane[p];
#pragma unroll
        for (int j = 0; j < 4; ++j) { s[j] += (double)v[j]; s[4 + j] += (double)v[j] * (double)v[j]; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double v = s[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8)
        partial[((size_t)blockIdx.x * c4 + cg) * 8 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void train_stats_partial_kernel(const f32x4 *y, int g0, int npix, double *partial)
{
    train_stats_partial_body(y, g0, npix, partial);
}

// Totals of the kTrainSlabs partial rows of channel group cg (8 doubles each: what the partial kernels wrote), formed
// by every block that needs them instead of a one-block "finish" launch per layer (two of the six small kernels a layer
// used to cost): lane b of the calling wave takes row b, an xor butterfly adds them - a fixed tree, every lane and
// every block get bit-identical totals.
static_assert(kTrainSlabs == 64, "one partial row per lane");
__device__ __forceinline__ void train_group_totals(const double *partial, int c4, int cg, double (&tot)[8])
{
    const double *row = partial + ((size_t)(threadIdx.x & 63) * c4 + cg) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double v = row[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        tot[j] = v;
    }
}

// ---- normalise + activation + channel dropout ----------------------------------------------------------------------
struct BnActArgs {
    const f32x4 *y;      // conv output planes (window at y_g0)
    f32x4 *out;          // result planes (window at out_g0)
    const f32x4 *dout;   // backward: gradient of `out`
    f32x4 *dy;           // backward: gradient of y
    const float *mean, *invstd;       // [c4 * 4] (identity when has_bn == 0)
    const float *gamma, *beta;        // [C] or NULL
    const float *drop;                // [C] per-channel Dropout2d scale (0 or 1 / (1 - p)) or NULL
    double *partial;                  // backward reduce: [slabs][c4][8]
    int y_g0, out_g0, dout_g0, dy_g0, c4, C, npix, act, has_bn, training;
    float scale;                      // output scale of the last layer (tanh(.) * output_scale)
    // forward with BatchNorm: statistics are finished in the kernel's prologue (train_group_totals of `partial`, or the
    // running statistics in eval mode); block column 0 publishes mean / invstd and updates the running statistics
    float *mean_out, *invstd_out, *running_mean, *running_var;
    float momentum, eps;
    // backward: block column 0 publishes the parameter gradients (added to what is there when `accumulate`)
    float *dgamma, *dbeta, *dbias;
    float *sum_dy;                    // backward, optional: [C] per-channel sums of dy (0 under batch statistics), plain store
    // backward, optional (the whole-net executor): dy is STORED multiplied by a power of two, so that the split-fp16
    // backward-data convolution and weight gradient see operands inside the fp16 range with all their bits; the consumers
    // divide again (exact).  The factor is derived IN THIS PASS from a guaranteed bound on |dy|, not from the previous pass:
    //   dy = gamma invstd (dz - mean(dz) - xhat mean(dz xhat))  =>  |dy| <= |gamma invstd| max|dz| (2 + max|xhat|^2)
    // (without batch statistics: |gamma invstd| max|dz|).  train_bn_bwd_reduce_kernel, which reads every dz and xhat anyway,
    // leaves  A_c = |gamma_c invstd_c| max|dz_c|  and  X_c = max|xhat_c|  in bnd[c] / bnd[bnd_stride + c] (atomicMax on the
    // bits of non-negative floats: kTrainSlabs arrivals per word); train_bn_bwd_apply_kernel turns them into the power of
    // two that puts the bound into [2^13, 2^14) and publishes it in *dy_scale_out.  No lag, no headroom to outgrow, nothing
    // to guard: a gradient of any magnitude is in range by construction (round 3 used the previous pass's maximum with 12
    // binades of headroom - a larger jump turned dy into +-inf halves and NaN sums that no guard could see).
    unsigned *bnd;
    int bnd_stride;
    float *dy_scale_out;
    int accumulate;
};

__device__ __forceinline__ float train_act(float z, int act)
{
    if (act == OJF_ACT_RELU) return z > 0.0f ? z : (z != z ? z : 0.0f);
    if (act == OJF_ACT_LEAKY) return z > 0.0f ? z : 0.01f * z;
    if (act == OJF_ACT_TANH) return tanhf(z);
    return z;
}
__device__ __forceinline__ float train_act_grad(float z, int act)
{
    if (act == OJF_ACT_RELU) return z > 0.0f ? 1.0f : 0.0f;
    if (act == OJF_ACT_LEAKY) return z > 0.0f ? 1.0f : 0.01f;
    if (act == OJF_ACT_TANH) { const float t = tanhf(z); return 1.0f - t * t; }
    return 1.0f;
}

// per-lane channel constants of group cg: (scale, shift) with z = y * scale + shift, drop, gamma * invstd
__device__ __forceinline__ void train_channel_consts(const BnActArgs &a, int cg, f32x4 &mu, f32x4 &is, f32x4 &ga, f32x4 &be, f32x4 &dr)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * cg + j;
        const bool real = c < a.C;
        mu[j] = (a.has_bn && a.mean) ? a.mean[c] : 0.0f;  // (forward: overwritten from the prologue's statistics)
        is[j] = real ? ((a.has_bn && a.invstd) ? a.invstd[c] : 1.0f) : 0.0f;
        ga[j] = real ? (a.gamma ? a.gamma[c] : 1.0f) : 0.0f;
        be[j] = real ? (a.beta ? a.beta[c] : 0.0f) : 0.0f;
        dr[j] = real ? (a.drop ? a.drop[c] : 1.0f) : 0.0f;
    }
}

// Up to four units of identical shape run as one launch (blockIdx.z): the four branches of a VortexPooling
// share_scale: the units' dy tensors are consumed as ONE stacked tensor (the branch entries) - one common factor
struct BnGroup { BnActArgs g[4]; int share_scale; };

__global__ __launch_bounds__(256) void train_stats_group_kernel(const BnGroup grp)
{
    const BnActArgs &a = grp.g[blockIdx.z];
    if (!(a.has_bn && a.training)) return;
    train_stats_partial_body(a.y, a.y_g0, a.npix, a.partial);
}

__global__ __launch_bounds__(256) void train_bn_act_fwd_kernel(const BnGroup grp)
{
    const BnActArgs &a = grp.g[blockIdx.z];
    const int cg = blockIdx.y;
    __shared__ float stat[8];  // mean[4], invstd[4] of this group
    // the first three loads of the streaming loop are requested BEFORE the statistics are finished (a chain of dependent
    // loads, shuffles and a barrier in front of them cost every one of ~30 launches per pass 2-3 us)
    const f32x4 *yp = a.y + (size_t)(a.y_g0 + cg) * a.npix;
    const int stride = gridDim.x * blockDim.x;
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool first3 = p + 2 * stride < a.npix;
    f32x4 py0{0.f, 0.f, 0.f, 0.f}, py1 = py0, py2 = py0;
    if (first3) { py0 = yp[p]; py1 = yp[p + stride]; py2 = yp[p + 2 * stride]; }
    if (a.has_bn) {
        if (threadIdx.x < 64) {
            double tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (a.training) train_group_totals(a.partial, a.c4, cg, tot);
            if (threadIdx.x < 4) {
                const int j = threadIdx.x, c = 4 * cg + j;
                float m = 0.0f, is = 0.0f;  // padding channels stay exactly zero
                if (c < a.C && !a.training) {
                    m = a.running_mean[c];
                    is = 1.0f / sqrtf(a.running_var[c] + a.eps);
                } else if (c < a.C) {
                    const double n = (double)a.npix, md = tot[j] / n;
                    double var = tot[4 + j] / n - md * md;
                    var = var < 0.0 ? 0.0 : var;
                    m = (float)md;
                    is = (float)(1.0 / sqrt(var + (double)a.eps));
                    if (blockIdx.x == 0) {
                        // nn.BatchNorm2d: running = (1 - momentum) * running + momentum * batch (variance: the unbiased estimate)
                        a.running_mean[c] = (1.0f - a.momentum) * a.running_mean[c] + a.momentum * m;
                        const double unbiased = a.npix > 1 ? var * n / (n - 1.0) : var;
                        a.running_var[c] = (1.0f - a.momentum) * a.running_var[c] + a.momentum * (float)unbiased;
                    }
                }
                stat[j] = m; stat[4 + j] = is;
                if (blockIdx.x == 0) { a.mean_out[c] = m; a.invstd_out[c] = is; }
            }
        }
        __syncthreads();
    }
    f32x4 mu, is, ga, be, dr;
    train_channel_consts(a, cg, mu, is, ga, be, dr);
    if (a.has_bn) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { mu[j] = stat[j]; is[j] = 4 * cg + j < a.C ? stat[4 + j] : 0.0f; }
    }
    f32x4 *op = a.out + (size_t)(a.out_g0 + cg) * a.npix;
    auto one = [&](const f32x4 &y) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (y[j] - mu[j]) * is[j];
            const float z = xh * ga[j] + be[j];
            o[j] = 4 * cg + j < a.C ? train_act(z, a.act) * a.scale * dr[j] : 0.0f;
        }
        return o;
    };
    if (first3) {
        op[p] = one(py0); op[p + stride] = one(py1); op[p + 2 * stride] = one(py2);
        p += 3 * stride;
    }
    for (; p + 2 * stride < a.npix; p += 3 * stride) {  // three loads in flight per lane
        const f32x4 y0 = yp[p], y1 = yp[p + stride], y2 = yp[p + 2 * stride];
        op[p] = one(y0); op[p + stride] = one(y1); op[p + 2 * stride] = one(y2);
    }
    for (; p < a.npix; p += stride) op[p] = one(yp[p]);
}

// dz = dout * scale * drop * act'(z); partial sums of dz and dz * xhat per channel (fp64, fixed order)
__global__ __launch_bounds__(256) void train_bn_bwd_reduce_kernel(const BnGroup grp)
{
    const BnActArgs &a = grp.g[blockIdx.z];
    __shared__ double red[4][8];
    const int cg = blockIdx.y;
    f32x4 mu, is, ga, be, dr;
    train_channel_consts(a, cg, mu, is, ga, be, dr);
    const int per = (a.npix + kTrainSlabs - 1) / kTrainSlabs;
    const int p0 = blockIdx.x * per, p1 = min(a.npix, p0 + per);
    const f32x4 *yp = a.y + (size_t)(a.y_g0 + cg) * a.npix;
    const f32x4 *gp = a.dout + (size_t)(a.dout_g0 + cg) * a.npix;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float mx[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // max |dz|, max |xhat| per channel (the bound behind dy's factor)
    auto add = [&](const f32x4 &y, const f32x4 &g) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (y[j] - mu[j]) * is[j];
            const float z = xh * ga[j] + be[j];
            const float dz = g[j] * a.scale * dr[j] * train_act_grad(z, a.act);
            s[j] += (double)dz;
            s[4 + j] += (double)dz * (double)xh;
            mx[j] = fmaxf(mx[j], fabsf(dz));
            mx[4 + j] = fmaxf(mx[4 + j], fabsf(xh));
        }
    };
    int p = p0 + threadIdx.x;
    for (; p + 768 < p1; p += 1024) {  // eight loads in flight per lane, sums in the order of a plain loop
        const f32x4 y4[4] = {yp[p], yp[p + 256], yp[p + 512], yp[p + 768]};
        const f32x4 g4[4] = {gp[p], gp[p + 256], gp[p + 512], gp[p + 768]};
#pragma unroll
        for (int u = 0; u < 4; ++u) add(y4[u], g4[u]);
    }
    for (; p < p1; p += 256) add(yp[p], gp[p]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double v = s[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8)
        a.partial[((size_t)blockIdx.x * a.c4 + cg) * 8 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (a.bnd) {
        __shared__ float redm[4][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = mx[j];
            for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
            if ((threadIdx.x & 63) == 0) redm[threadIdx.x >> 6][j] = v;
        }
        __syncthreads();
        if (threadIdx.x < 8) {
            const int j = threadIdx.x & 3, c = 4 * cg + j;
            float v = fmaxf(fmaxf(redm[0][threadIdx.x], redm[1][threadIdx.x]), fmaxf(redm[2][threadIdx.x], redm[3][threadIdx.x]));
            if (threadIdx.x < 4) v *= fabsf(ga[j] * is[j]);  // (the per-lane constants are the same in every lane)
            // (an infinite maximum orders above every finite one; a NaN never wins an fmaxf: NaN gradients are the
            // reference's NaN gradients, not a range event)
            if (c < a.C && v > 0.0f) atomicMax(a.bnd + (threadIdx.x < 4 ? 0 : a.bnd_stride) + c, __float_as_uint(v));
        }
    }
}

// the power of two that brings `bound` into [2^13, 2^14) (1 for a zero or non-finite bound)
__device__ __forceinline__ float train_dy_factor(float bound)
{
    if (!(bound > 0.0f) || !(bound < 3.0e38f)) return 1.0f;
    int e = 0;
    (void)frexpf(bound, &e);  // bound = f 2^e, f in [0.5, 1)
    int k = 14 - e;
    k = k > 100 ? 100 : (k < -100 ? -100 : k);
    return ldexpf(1.0f, k);
}

__global__ __launch_bounds__(256) void train_bn_bwd_apply_kernel(const BnGroup grp)
{
    const BnActArgs &a = grp.g[blockIdx.z];
    const int cg = blockIdx.y;
    f32x4 mu, is, ga, be, dr;
    train_channel_consts(a, cg, mu, is, ga, be, dr);
    // (the first six loads of the streaming loop go out before the reductions are finished and the bound is scanned: see
    // train_bn_act_fwd_kernel)
    const f32x4 *yp = a.y + (size_t)(a.y_g0 + cg) * a.npix;
    const f32x4 *gp = a.dout + (size_t)(a.dout_g0 + cg) * a.npix;
    const int stride = gridDim.x * blockDim.x;
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool first3 = p + 2 * stride < a.npix;
    f32x4 py0{0.f, 0.f, 0.f, 0.f}, py1 = py0, py2 = py0, pg0 = py0, pg1 = py0, pg2 = py0;
    if (first3) {
        py0 = yp[p]; py1 = yp[p + stride]; py2 = yp[p + 2 * stride];
        pg0 = gp[p]; pg1 = gp[p + stride]; pg2 = gp[p + 2 * stride];
    }
    // the two reductions are finished here (see train_group_totals); block column 0 publishes the parameter gradients
    __shared__ float means[8];
    if (threadIdx.x < 64) {
        double tot[8];
        train_group_totals(a.partial, a.c4, cg, tot);
        if (threadIdx.x < 4) {
            const int j = threadIdx.x, c = 4 * cg + j;
            const bool batch = a.has_bn && a.training;
            means[j] = batch ? (float)(tot[j] / (double)a.npix) : 0.0f;          // mean(dz)
            means[4 + j] = batch ? (float)(tot[4 + j] / (double)a.npix) : 0.0f;  // mean(dz * xhat)
            if (blockIdx.x == 0 && c < a.C) {
                if (a.dgamma) a.dgamma[c] = (a.accumulate ? a.dgamma[c] : 0.0f) + (float)tot[4 + j];
                if (a.dbeta) a.dbeta[c] = (a.accumulate ? a.dbeta[c] : 0.0f) + (float)tot[j];
                if (a.sum_dy) a.sum_dy[c] = batch ? 0.0f : (float)(tot[j] * (double)(a.has_bn ? (a.gamma ? a.gamma[c] : 1.0f) * a.invstd[c] : 1.0f));
                if (a.dbias) {
                    // sum_p dy: zero under batch statistics (the normalisation removes the mean), gamma * invstd * sum(dz) otherwise
                    const float gi = a.has_bn ? (a.gamma ? a.gamma[c] : 1.0f) * a.invstd[c] : 1.0f;
                    a.dbias[c] = (a.accumulate ? a.dbias[c] : 0.0f) + (batch ? 0.0f : (float)(tot[j] * (double)gi));
                }
            }
        }
    }
    __syncthreads();
    f32x4 m1, m2;
#pragma unroll
    for (int j = 0; j < 4; ++j) { m1[j] = means[j]; m2[j] = means[4 + j]; }
    f32x4 *dp = a.dy + (size_t)(a.dy_g0 + cg) * a.npix;
    float dys = 1.0f;
    if (a.bnd) {  // this pass's factor from the bound the reduce launch left (the same value in every block of the scale group)
        __shared__ float bw[4];
        const int n_units = grp.share_scale ? (int)gridDim.z : 1, per = 4 * a.c4;
        float b = 0.0f;
        // (strided: a wide net - ojf_trainer_create takes widths up to 1024 - has more bound words than the block has threads)
        for (int i = threadIdx.x; i < n_units * per; i += blockDim.x) {
            const int u = i / per, c = i - u * per;
            const BnActArgs &o = grp.g[grp.share_scale ? u : (int)blockIdx.z];
            if (c < o.C) {
                const float A = __uint_as_float(o.bnd[c]), X = __uint_as_float(o.bnd[o.bnd_stride + c]);
                float bi = (o.has_bn && o.training) ? A * (2.0f + X * X) : A;
                if (bi != bi) bi = 3.4e38f;  // (inf * 0)
                b = fmaxf(b, bi);
            }
        }
        for (int off = 32; off > 0; off >>= 1) b = fmaxf(b, __shfl_xor(b, off, 64));
        if ((threadIdx.x & 63) == 0) bw[threadIdx.x >> 6] = b;
        __syncthreads();
        dys = train_dy_factor(fmaxf(fmaxf(bw[0], bw[1]), fmaxf(bw[2], bw[3])));
        if (a.dy_scale_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.dy_scale_out = dys;
    }
    auto one = [&](const f32x4 &y, const f32x4 &g) {
        f32x4 d;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (y[j] - mu[j]) * is[j];
            const float z = xh * ga[j] + be[j];
            const float dz = g[j] * a.scale * dr[j] * train_act_grad(z, a.act);
            const float v = ga[j] * is[j] * (dz - m1[j] - xh * m2[j]);  // m1 = m2 = 0 without batch statistics
            d[j] = v * dys;
        }
        return d;
    };
    if (first3) {
        dp[p] = one(py0, pg0); dp[p + stride] = one(py1, pg1); dp[p + 2 * stride] = one(py2, pg2);
        p += 3 * stride;
    }
    for (; p + 2 * stride < a.npix; p += 3 * stride) {  // six loads in flight per lane
        const f32x4 y0 = yp[p], y1 = yp[p + stride], y2 = yp[p + 2 * stride];
        const f32x4 g0 = gp[p], g1 = gp[p + stride], g2 = gp[p + 2 * stride];
        dp[p] = one(y0, g0); dp[p + stride] = one(y1, g1); dp[p + 2 * stride] = one(y2, g2);
    }
    for (; p < a.npix; p += stride) dp[p] = one(yp[p], gp[p]);
}

// ---- weight gradient -----------------------------------------------------------------------------------------------
// dW[oc][ic][tap] = sum_p dy[oc][p] * x[ic][p + offset(tap)] (zero outside the image) on the fp32 MFMA, K = pixels.
// Partial sums per pixel slab go to `partial`; wgrad_reduce_kernel adds the slabs in order and writes torch's
// [OC][IC][k][k] layout (physical input channels un-slotted).  (Round 2 started with a register-tiled fp32 FMA kernel -
// 4 x 4 (oc, ic) tile per thread, 40-80 us per layer; the MFMA form takes 12-36 us on the same layers.)
struct WgradArgs {
    const f32x4 *x;   // input planes of the forward conv (window at x_g0, c4_in groups)
    const f32x4 *dy;  // gradient planes of its output (window at dy_g0, c4_out groups)
    float *partial;   // [slabs][taps][ocp][icp], ocp / icp = channel counts rounded up to 32
    int x_g0, c4_in, dy_g0, c4_out, h, w, npix, taps, dil, slabs, ocp, icp;
    int *ovf;  // split-fp16 form: range-guard flag for dy where no backward-data convolution checks it (else NULL)
};

// One wave (= one block) = one 32 x 32 (oc, ic) tile of ONE tap over one
// pixel slab, D += A * B with v_mfma_f32_32x32x2_f32, K = 2 pixels per instruction: lane (r = lane % 32, k = lane / 32)
// supplies A[r][k] = dy[oc0 + r][p + k] and B[k][r] = x[ic0 + r][p + k + tap offset].  The C4 planes hold 4 channels
// per 16 bytes, so those scalars are transposed through LDS: per 64-pixel chunk every lane fetches ITS pixel's eight
// float4 of dy and of x (1 KB contiguous per wave instruction; taps outside the image, channels outside the tensor and
// pixels outside the slab become zeros here) and writes them as a [pixel][32 channels] row (pitch 36 floats:
// conflict-free float4 writes), then 32 K steps read one float per lane and operand.  (Fetching the scalars straight
// from global memory - 16 sixteen-byte segments per wave load - ran at a quarter of the MFMA rate: the L1 address
// path, not the pipe, was the bound.)  Same `partial` layout as the VALU kernel ([slab][tap][ocp][icp], ocp / icp
// multiples of 32), same fixed-order reduction afterwards.
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kWgChunk = 64, kWgPitch = 36;

struct WgradGroup { WgradArgs g[4]; int tiles; };  // blockIdx.y = unit * tiles + (oc, ic) tile

// F16: split-fp16 form (v_mfma_f32_32x32x16_f16, three per 16 pixels: dy_hi x_hi + dy_hi x_lo + dy_lo x_hi, fp32 accumulate)
// for passes whose dy carries its power-of-two factor (the trainer's second backward pass on) - the matrix pipe's share of a
// 64-pixel chunk drops from 32 x 64 to 12 x 32 cycles.  Same staging; the transposed LDS reads fetch EIGHT consecutive
// pixels of the lane's channel (K = 8 k .. 8 k + 7 of a 16-pixel step, the same pixels for A and for B) and are split in
// registers.  x is an activation the forward convolution already split (inside the fp16 range by its guard); dy is
// guarded by the backward-data convolution that reads the same planes, or here (a.ovf) where there is none.
template <bool F16>
__global__ __launch_bounds__(64) void train_wgrad_mfma_kernel(const WgradGroup grp, unsigned w_magic)
{
    __shared__ __attribute__((aligned(16))) float tile[2][kWgChunk * kWgPitch];
    const int unit = blockIdx.y / grp.tiles, tile_i = blockIdx.y - unit * grp.tiles;
    const WgradArgs &a = grp.g[unit];
    const int lane = threadIdx.x, r = lane & 31, k = lane >> 5;
    const int n_it = a.icp / 32;
    const int ot = tile_i / n_it, it = tile_i - ot * n_it;
    const int tap = blockIdx.z;
    int dyo = 0, dxo = 0;
    if (a.taps == 9) { dyo = (tap / 3 - 1) * a.dil; dxo = (tap % 3 - 1) * a.dil; }
    const int per = ((a.npix + a.slabs - 1) / a.slabs + 1) & ~1;  // even: a K step never straddles two slabs
    const int p0 = blockIdx.x * per, p1 = min(a.npix, p0 + per);
    const int shift = dyo * a.w + dxo;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
    f32x4 dv[8], xv[8];
    float gmax = 0.0f;
    // buffer loads: a lane outside the slab / a tap outside the image gets an offset beyond the descriptor's range and
    // reads zeros, and so does a channel group outside the tensor - no per-load branches (as plain predicated loads the
    // sixteen fetches of a chunk were sixteen exec-mask regions, ~130 VALU + ~240 scalar instructions)
    const int n_og = min(8, a.c4_out - ot * 8), n_ig = min(8, a.c4_in - it * 8);
    const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<f32x4 *>(a.dy + (size_t)(a.dy_g0 + ot * 8) * a.npix), 0, n_og * a.npix * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<f32x4 *>(a.x + (size_t)(a.x_g0 + it * 8) * a.npix), 0, n_ig * a.npix * 16, 0x00020000);
    const int plane = a.npix * 16;
    auto fetch = [&](int pc) {  // this lane's pixel of the chunk at pc: its eight channel groups of dy and of x
        const int p = pc + lane;
        const int py = fast_div(p, a.w, w_magic), px = p - py * a.w;
        const bool in = p < p1;
        const bool tap_ok = in && (unsigned)(py + dyo) < (unsigned)a.h && (unsigned)(px + dxo) < (unsigned)a.w;
        const unsigned od = in ? (unsigned)p * 16u : 0x80000000u, ox = tap_ok ? (unsigned)(p + shift) * 16u : 0x80000000u;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            // (the plane offset rides in the per-lane offset, which the range check sees: groups past the tensor read zeros too)
            dv[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_dy, od + (unsigned)(g * plane), 0, 0));
            xv[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, ox + (unsigned)(g * plane), 0, 0));
        }
    };
    fetch(p0);
    for (int pc = p0; pc < p1; pc += kWgChunk) {
        __syncthreads();  // (one wave per block: orders the previous chunk's reads before these writes)
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            *reinterpret_cast<f32x4 *>(&tile[0][lane * kWgPitch + 4 * g]) = dv[g];
            *reinterpret_cast<f32x4 *>(&tile[1][lane * kWgPitch + 4 * g]) = xv[g];
        }
        if constexpr (F16)
            if (a.ovf) {
#pragma unroll
                for (int g = 0; g < 8; ++g) gmax = guard_max(gmax, dv[g]);
            }
        __syncthreads();
        fetch(pc + kWgChunk);  // the next chunk travels while this one is multiplied (past the slab: all zeros, no traffic)
        if constexpr (F16) {
            // a register block = one 16-pixel K step: 8 + 8 transposed reads, two splits, three MFMAs
            float av[2][8], bv[2][8];
            auto read_step = [&](int s, float (&ar)[8], float (&br)[8]) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    ar[u] = tile[0][(16 * s + 8 * k + u) * kWgPitch + r];
                    br[u] = tile[1][(16 * s + 8 * k + u) * kWgPitch + r];
                }
            };
            read_step(0, av[0], bv[0]);
#pragma unroll
            for (int s = 0; s < kWgChunk / 16; ++s) {
                if (s + 1 < kWgChunk / 16) read_step(s + 1, av[(s + 1) & 1], bv[(s + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                const float(&ar)[8] = av[s & 1];
                const float(&br)[8] = bv[s & 1];
                f16x8 dh, dl, xh, xl;
                split_f16(f32x4{ar[0], ar[1], ar[2], ar[3]}, f32x4{ar[4], ar[5], ar[6], ar[7]}, dh, dl);
                split_f16(f32x4{br[0], br[1], br[2], br[3]}, f32x4{br[4], br[5], br[6], br[7]}, xh, xl);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dl, xh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh, xl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh, xh, acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            // operands of eight K steps per register block; the next block's LDS reads are issued before this block's
            // MFMAs (read -> wait -> 2 MFMAs, as the compiler schedules the plain loop, exposes the LDS latency 16 times)
            float av[2][8], bv[2][8];
            auto read_block = [&](int blk, float (&ar)[8], float (&br)[8]) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    ar[u] = tile[0][(2 * (8 * blk + u) + k) * kWgPitch + r];
                    br[u] = tile[1][(2 * (8 * blk + u) + k) * kWgPitch + r];
                }
            };
            read_block(0, av[0], bv[0]);
#pragma unroll
            for (int blk = 0; blk < kWgChunk / 16; ++blk) {
                if (blk + 1 < kWgChunk / 16) read_block(blk + 1, av[(blk + 1) & 1], bv[(blk + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise sinks every read next to its MFMA again)
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[blk & 1][u], bv[blk & 1][u], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if constexpr (F16)
        if (a.ovf && gmax > 65504.0f) guard_raise(a.ovf, 1);
    // D layout: acc[v] = D[i][j], j = lane % 32 (ic), i = 8 * (v / 4) + 4 * (lane / 32) + v % 4 (oc)
    float *dst = a.partial + (((size_t)blockIdx.x * a.taps + tap) * a.ocp + (size_t)ot * 32) * a.icp + (size_t)it * 32 + r;
#pragma unroll
    for (int v = 0; v < 16; ++v) dst[(size_t)(8 * (v / 4) + 4 * k + (v % 4)) * a.icp] = acc[v];
}

// (Round 3 tried a row-merged form for the 3x3 layers - one wave = the three taps of a kernel row, dy staged once per three
// taps, x once per 64 + 2 d pixel band with per-pixel tap masks at read time, a third of the traffic through L2: correct,
// but 174 against 191 frames/s for the training step - a third of the waves with three accumulators each hide the LDS
// transposes worse than they save fetches.)
struct WgradReduceArgs {
    const float *partial;
    float *dw;  // [OC][IC][taps]
    int slabs, taps, ocp, icp, OC, IC, group, slot, c_in_phys;
    int accumulate;  // dw += (gradient accumulation over frames happens here instead of in a torch add per parameter)
    int oc_base;     // first row of `partial` that belongs to this weight tensor (stacked layers; else 0)
    int ic_base, ic_total;  // the gradient covers input channels [ic_base, ic_base + IC) of a tensor with ic_total of them
    const float *dy_scale;  // dy carried this power-of-two factor (NULL: none): the sums are divided by it
};
struct WgradReduceGroup { WgradReduceArgs g[4]; };  // blockIdx.y = unit

// eight lanes per weight: lane `sub` adds slabs sub, sub + 8, ... in order, then a fixed xor tree joins the eight sums
__global__ __launch_bounds__(256) void train_wgrad_reduce_kernel(const WgradReduceGroup grp)
{
    const WgradReduceArgs &a = grp.g[blockIdx.y];
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i = t >> 3;
    const int sub = (int)(t & 7);
    const long total = (long)a.taps * a.OC * a.c_in_phys;
    const bool live = i < total;
    const long ii = live ? i : 0;
    const int icp_i = (int)(ii % a.c_in_phys);
    const long r = ii / a.c_in_phys;
    const int oc = (int)(r % a.OC), tap = (int)(r / a.OC);
    float s = 0.0f;
    if (live)
        for (int b = sub; b < a.slabs; b += 8) s += a.partial[(((size_t)b * a.taps + tap) * a.ocp + a.oc_base + oc) * a.icp + icp_i];
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 1, 64);
    if (!live || sub) return;
    if (a.dy_scale) s /= *a.dy_scale;  // exact: a power of two
    const int ic = train_unslot(icp_i, a.group, a.slot, a.IC);
    if (ic >= 0) {
        float *d = a.dw + ((size_t)oc * a.ic_total + a.ic_base + ic) * a.taps + tap;
        *d = a.accumulate ? *d + s : s;
    }
}

// nn.AvgPool2d(3, stride 1, padding 1), count_include_pad: out = (sum of the 3x3 neighbourhood inside the image) / 9.  The
// operator is symmetric, so its backward pass is the same kernel applied to the gradient.
__global__ __launch_bounds__(256) void train_avgpool3_kernel(const f32x4 *in, f32x4 *out, int h, int w)
{
    const int npix = h * w;
    const f32x4 *ip = in + (size_t)blockIdx.y * npix;
    f32x4 *op = out + (size_t)blockIdx.y * npix;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        const int y = p / w, x = p - y * w;
        f32x4 s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
                if ((unsigned)(y + dy) < (unsigned)h && (unsigned)(x + dx) < (unsigned)w) s += ip[(y + dy) * w + x + dx];
        op[p] = s / 9.0f;
    }
}

// ---- small kernels of the executor ---------------------------------------------------------------------------------
struct PackInArgs {
    const float *src[4];  // NCHW sources [n_i][npix]
    int nch[4];
    int n_src, c4, npix;
    f32x4 *dst;           // planes [c4][npix]
};

__global__ __launch_bounds__(256) void train_pack_input_kernel(const PackInArgs a)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.npix) return;
    const int cg = blockIdx.y;
    f32x4 v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int l = 4 * cg + j;
        for (int s = 0; s < a.n_src; ++s) {
            if (l < a.nch[s]) { v[j] = a.src[s][(size_t)l * a.npix + p]; break; }
            l -= a.nch[s];
        }
    }
    a.dst[(size_t)cg * a.npix + p] = v;
}

// planes [c4][npix] <-> NCHW [C][npix] (est out / d est in); channels >= C are dropped / zero
__global__ __launch_bounds__(256) void train_planes_to_nchw_kernel(const f32x4 *pl, int c4, int C, int npix, float *dst)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const f32x4 v = pl[(size_t)blockIdx.y * npix + p];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * (int)blockIdx.y + j < C) dst[(size_t)(4 * blockIdx.y + j) * npix + p] = v[j];
}

__global__ __launch_bounds__(256) void train_nchw_to_planes_kernel(const float *src, int C, int npix, f32x4 *pl)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    f32x4 v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * (int)blockIdx.y + j < C) v[j] = src[(size_t)(4 * blockIdx.y + j) * npix + p];
    pl[(size_t)blockIdx.y * npix + p] = v;
}

// out[group g] = P^lv(in[group g]) (+ bias of the branch), lv = g / sl4: branch i of a VortexPooling sees i successive
// nn.AvgPool2d(3, 1, 1) (count_include_pad: zeros outside the image, divide by 9 - every level zero-pads anew).  One block =
// one 32 x 8 pixel tile of one channel group, the intermediate levels live in LDS with a shrinking halo.  The operator is
// symmetric, so the backward pass is the same kernel on the gradient (without bias).
struct TrainPyramidArgs {
    const f32x4 *in;
    f32x4 *out;
    const float *bias[4];  // per branch: [OC] logical, or NULL
    int h, w, sl4, OC;
};
constexpr int kTpW = 32, kTpH = 8, kTpStride = kTpW + 6;

__global__ __launch_bounds__(256) void train_pyramid_kernel(const TrainPyramidArgs a)
{
    __shared__ f32x4 buf[2][kTpStride * (kTpH + 6)];
    const int g = blockIdx.y, lv = g / a.sl4, cg = g - lv * a.sl4;
    const int tiles_x = (a.w + kTpW - 1) / kTpW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kTpW, y0 = ty * kTpH, npix = a.h * a.w;
    const f32x4 *plane = a.in + (size_t)g * npix;
    const f32x4 zero{0.f, 0.f, 0.f, 0.f};
    f32x4 b = zero;
    if (a.bias[lv])
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * cg + j < a.OC) b[j] = a.bias[lv][4 * cg + j];
    if (lv == 0) {
        const int ly = threadIdx.x / kTpW, lx = threadIdx.x - ly * kTpW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy < a.h && gx < a.w) a.out[(size_t)g * npix + gy * a.w + gx] = plane[gy * a.w + gx] + b;
        return;
    }
    {
        const int W0 = kTpW + 2 * lv, H0 = kTpH + 2 * lv;
        for (int i = threadIdx.x; i < W0 * H0; i += 256) {
            const int ly = i / W0, lx = i - ly * W0;
            const int gy = y0 - lv + ly, gx = x0 - lv + lx;
            const bool in = (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
            buf[0][ly * kTpStride + lx] = in ? plane[gy * a.w + gx] : zero;
        }
    }
    __syncthreads();
    for (int l = 1; l <= lv; ++l) {
        const int halo = lv - l;
        const int Wl = kTpW + 2 * halo, Hl = kTpH + 2 * halo;
        const f32x4 *src = buf[(l - 1) & 1];
        for (int i = threadIdx.x; i < Wl * Hl; i += 256) {
            const int ly = i / Wl, lx = i - ly * Wl;
            const int gy = y0 - halo + ly, gx = x0 - halo + lx;
            const bool in = (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
            f32x4 s = zero;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) s += src[(ly + dy) * kTpStride + lx + dx];
            s = s / 9.0f;
            if (l < lv) buf[l & 1][ly * kTpStride + lx] = in ? s : zero;
            else if (in) a.out[(size_t)g * npix + gy * a.w + gx] = s + b;
        }
        __syncthreads();
    }
}

// ---- global-average branch of a VortexPooling (modules/model.py:103-109,146): AdaptiveAvgPool2d(1) -> 1x1 conv ->
// up-sampling of the 1x1 map (a broadcast) -> BatchNorm2d.  The BatchNorm sees a constant map: with batch statistics its
// output is beta (variance 0), nothing upstream receives a gradient, running_mean moves towards the map's value and
// running_var towards 0; with running statistics it is an affine map of g = W mean(x) + b and gradients flow to W, b,
// gamma, beta and (as a per-channel constant over all pixels) to x.  One block does the vector work.
struct GaveTrainArgs {
    const double *partial;   // [slabs][c4_in][8]: channel sums of x (forward) / of d cat[gave slot] (backward)
    int c4_in, c4_out, IC, OC, group, slot, npix, training, accumulate;
    float momentum, eps;
    const float *W, *b, *gamma, *beta;
    float *running_mean, *running_var;
    float *pooled, *xhat, *gis;  // saved for backward: [4 c4_in] mean of x per physical channel, [OC] x-hat, [OC] gamma * invstd
    float *vec;                  // forward: [4 c4_out] value of the branch's constant map (padding channels 0)
    float *dW, *db, *dgamma, *dbeta;
    float *dpooled;              // backward (eval): [4 c4_in] per-channel constant added to d x
    // The branch's constant map is input channels [0, OC) of the VortexPooling's final 1x1 convolution (weights Wf
    // [OCf][ICf_total], bias bf): over a constant map that convolution is a per-frame BIAS, Wf[:, :OC] vec - so the map is
    // never materialised, the final convolution reads the four branch slots only, and backward needs just the channel
    // sums of the final convolution's dy: d vec = Wf[:, :OC]^T sum_dy,  d Wf[:, :OC] = sum_dy (x) vec.
    const float *Wf, *bf;
    int OCf, ICf_total, accumulate_f;
    float *bias_eff;             // forward: [OCf] bf + Wf[:, :OC] vec -> the final unit's packed bias
    const float *sum_dy;         // backward: [OCf]
    float *dWf;                  // backward: the final convolution's weight gradient (columns [0, OC) written here)
};

// sum of the kTrainSlabs partial rows of physical channel ch, by one wave (lane b takes row b; fixed xor tree)
__device__ __forceinline__ double gave_slab_sum(const double *partial, int c4, int ch)
{
    double v = partial[((size_t)(threadIdx.x & 63) * c4 + (ch >> 2)) * 8 + (ch & 3)];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

constexpr int kGaveThreads = 1024, kGaveMaxC = 1024;

__global__ __launch_bounds__(kGaveThreads) void train_gave_fwd_kernel(const GaveTrainArgs a)
{
    __shared__ float pooled[kGaveMaxC], vecs[kGaveMaxC];
    const int wave = threadIdx.x >> 6, nw = kGaveThreads / 64;
    for (int ch = wave; ch < 4 * a.c4_in; ch += nw) {
        const float m = (float)(gave_slab_sum(a.partial, a.c4_in, ch) / (double)a.npix);
        if ((threadIdx.x & 63) == 0) { pooled[ch] = m; a.pooled[ch] = m; }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 4 * a.c4_out; o += kGaveThreads) {
        float vec = 0.0f;
        if (o < a.OC) {
            float g = a.b ? a.b[o] : 0.0f;
            for (int l = 0; l < a.IC; ++l) g = fmaf(a.W[(size_t)o * a.IC + l], pooled[(l / a.group) * a.slot + l % a.group], g);
            const float ga = a.gamma ? a.gamma[o] : 1.0f, be = a.beta ? a.beta[o] : 0.0f;
            if (a.training) {
                a.running_mean[o] = (1.0f - a.momentum) * a.running_mean[o] + a.momentum * g;
                a.running_var[o] = (1.0f - a.momentum) * a.running_var[o];
                a.xhat[o] = 0.0f;
                a.gis[o] = 0.0f;
                vec = be;
            } else {
                const float is = 1.0f / sqrtf(a.running_var[o] + a.eps);
                const float xh = (g - a.running_mean[o]) * is;
                a.xhat[o] = xh;
                a.gis[o] = ga * is;
                vec = xh * ga + be;
            }
        }
        a.vec[o] = vec;
        vecs[o] = vec;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < a.OCf; o += kGaveThreads) {  // the constant map's share of the final convolution = a bias
        float b = a.bf ? a.bf[o] : 0.0f;
        for (int c = 0; c < a.OC; ++c) b = fmaf(a.Wf[(size_t)o * a.ICf_total + c], vecs[c], b);
        a.bias_eff[o] = b;
    }
}

__global__ __launch_bounds__(kGaveThreads) void train_gave_bwd_kernel(const GaveTrainArgs a)
{
    __shared__ float dg[kGaveMaxC], sdy[kGaveMaxC];
    for (int o = threadIdx.x; o < a.OCf; o += kGaveThreads) sdy[o] = a.sum_dy[o];
    __syncthreads();
    for (int c = threadIdx.x; c < a.OC; c += kGaveThreads) {
        float dv = 0.0f;  // d vec = Wf[:, :OC]^T sum_dy
        for (int o = 0; o < a.OCf; ++o) dv = fmaf(a.Wf[(size_t)o * a.ICf_total + c], sdy[o], dv);
        if (a.dbeta) a.dbeta[c] = (a.accumulate ? a.dbeta[c] : 0.0f) + dv;
        if (a.dgamma) a.dgamma[c] = (a.accumulate ? a.dgamma[c] : 0.0f) + dv * a.xhat[c];
        const float d = dv * a.gis[c];  // 0 under batch statistics
        dg[c] = d;
        if (a.db) a.db[c] = (a.accumulate ? a.db[c] : 0.0f) + d;
    }
    __syncthreads();
    if (a.dW)
        for (int i = threadIdx.x; i < a.OC * a.IC; i += kGaveThreads) {
            const int o = i / a.IC, l = i - o * a.IC;
            a.dW[i] = (a.accumulate ? a.dW[i] : 0.0f) + dg[o] * a.pooled[(l / a.group) * a.slot + l % a.group];
        }
    if (a.dWf)
        for (int i = threadIdx.x; i < a.OCf * a.OC; i += kGaveThreads) {
            const int o = i / a.OC, c = i - o * a.OC;
            float *d = a.dWf + (size_t)o * a.ICf_total + c;
            *d = (a.accumulate_f ? *d : 0.0f) + sdy[o] * a.vec[c];
        }
    if (a.training) return;  // nothing flows back to x under batch statistics (dg == 0)
    for (int ch = threadIdx.x; ch < 4 * a.c4_in; ch += kGaveThreads) {
        const int s = ch / a.slot, in = ch - s * a.slot, l = s * a.group + in;
        float d = 0.0f;
        if (in < a.group && l < a.IC)
            for (int o = 0; o < a.OC; ++o) d = fmaf(a.W[(size_t)o * a.IC + l], dg[o], d);
        a.dpooled[ch] = d / (float)a.npix;
    }
}

// planes[g][p] = vec[4g .. 4g+3] (add != 0: +=)
__global__ __launch_bounds__(256) void train_bcast_planes_kernel(const float *vec, f32x4 *pl, int npix, int add)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const f32x4 v = *reinterpret_cast<const f32x4 *>(vec + 4 * blockIdx.y);
    f32x4 *d = pl + (size_t)blockIdx.y * npix + p;
    *d = add ? *d + v : v;
}

// ---- the frame step's glue around the net (modules/pipeline.py:104-135, utils/loss.py:65-103) -------------------------
// fused[r][k] = (max(w, 0) v + clamp(est, +-init)) / (max(w, 0) + 1) at pixel valid[r], sample k: the "weighted update"
// of pipeline.py:107-116 followed by the masking of :121-127, from the plane layout [P][n] into the API's rows [Nv][P].
struct FuseOutArgs {
    const float *est, *fv, *fw;  // [P][n]
    const long long *valid;      // [Nv] pixel indices
    float *rows;                 // forward: fused [Nv][P]; backward: d fused [Nv][P] (read)
    float *d_est;                // backward: [P][n], zeroed by the caller
    int n, P;
    long long n_valid;
    float init;
};

__global__ __launch_bounds__(256) void train_fuse_output_kernel(const FuseOutArgs a)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_valid) return;
    const long long p = a.valid[r];
    for (int k = 0; k < a.P; ++k) {
        const size_t i = (size_t)k * a.n + p;
        float w = a.fw[i];
        w = w < 0.0f ? 0.0f : w;                                        // pipeline.py:113-114
        float e = a.est[i];
        e = e < -a.init ? -a.init : (e > a.init ? a.init : e);           // :109-111 (NaN passes through like torch.clamp)
        a.rows[(size_t)r * a.P + k] = (w * a.fv[i] + e) / (w + 1.0f);   // :116
    }
}

__global__ __launch_bounds__(256) void train_fuse_output_bwd_kernel(const FuseOutArgs a)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_valid) return;
    const long long p = a.valid[r];
    for (int k = 0; k < a.P; ++k) {
        const size_t i = (size_t)k * a.n + p;
        float w = a.fw[i];
        w = w < 0.0f ? 0.0f : w;
        const float e = a.est[i];
        const bool pass = !(e < -a.init) && !(e > a.init);  // torch.clamp: the gradient passes inside the closed interval
        a.d_est[i] = pass ? a.rows[(size_t)r * a.P + k] / (w + 1.0f) : 0.0f;
    }
}

// FusionLoss (utils/loss.py:65-103): w1 mean|e - t| + w2 mean (e - t)^2 + w3 mean_j (1 - cos_j), where the cosine runs
// over the reference's RESHAPED sign tensors: column j of the [P, Nv] reinterpretation of the flat [Nv, P] array, i.e. the
// flat elements i Nv + j, i < P.  Thread j owns exactly those elements, so it also carries their share of the first two
// sums; per-block fp64 partial sums in a fixed tree, added in block order by the finishing block: bit-reproducible.
constexpr int kLossThreads = 256;
struct LossArgs {
    const float *est, *tgt;   // flat [Nv * P]
    long long nv;
    int P;
    float w1, w2, w3;
    double *partial;          // [blocks][4]
    float *loss;
    const float *grad_out;    // backward: d loss (device scalar)
    float *d_est;             // backward: [Nv * P]
    int blocks;
};

__device__ __forceinline__ float loss_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

__global__ __launch_bounds__(kLossThreads) void train_loss_partial_kernel(const LossArgs a)
{
    __shared__ double red[kLossThreads / 64][3];
    const long long j = (long long)blockIdx.x * kLossThreads + threadIdx.x;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (j < a.nv) {
        float dot = 0.0f, n1 = 0.0f, n2 = 0.0f;
        for (int i = 0; i < a.P; ++i) {
            const size_t f = (size_t)i * a.nv + j;
            const float e = a.est[f], t = a.tgt[f], d = e - t;
            s1 += (double)fabsf(d);
            s2 += (double)(d * d);
            const float se = loss_sign(e), st = loss_sign(t);
            dot += se * st; n1 += se * se; n2 += st * st;
        }
        s3 = (double)(1.0f - dot / sqrtf((n1 + 1e-12f) * (n2 + 1e-12f)));
    }
    double v[3] = {s1, s2, s3};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double x = v[q];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) a.partial[(size_t)blockIdx.x * 4 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(64) void train_loss_finish_kernel(const LossArgs a)
{
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < a.blocks; b += 64)  // lane l adds blocks l, l + 64, ... in order
        for (int q = 0; q < 3; ++q) s[q] += a.partial[(size_t)b * 4 + q];
    for (int q = 0; q < 3; ++q)
        for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_xor(s[q], off, 64);
    if (threadIdx.x == 0) {
        const double n = (double)a.nv * (double)a.P;
        *a.loss = (float)((double)a.w1 * s[0] / n + (double)a.w2 * s[1] / n + (double)a.w3 * s[2] / (double)a.nv);
    }
}

__global__ __launch_bounds__(256) void train_loss_bwd_kernel(const LossArgs a)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = a.nv * a.P;
    if (i >= total) return;
    const float g = *a.grad_out / (float)total;
    const float d = a.est[i] - a.tgt[i];
    a.d_est[i] = g * (a.w1 * loss_sign(d) + 2.0f * a.w2 * d);  // the sign-cosine term is piecewise constant
}

// ---- split-fp16 weights for the FORWARD convolutions, packed on the device -------------------------------------------
// The forward pass's convolutions see BatchNorm-scaled activations of order one: the inference path's split-fp16 arithmetic
// (three fp16 MFMAs per product block, fp32 accumulate, row-equilibrated weights: DESIGN.md 3.2) applies unchanged and runs
// the MFMA part 5.3x faster than the fp32-input instruction.  Gradients (tiny, of unbounded range) stay on fp32 MFMAs.
// Layout = finish()'s: [superstep][oc tile][hi | lo][lane] x 8 halfs, K entry G = 8 S + 2 (lane / 16) + j / 4.
struct Pack16Args {
    const float *w;        // [OC][ic_total][taps]
    float *rs;             // [n_ot * 16] power-of-two row scales (written by the row-max pass)
    float *rinv;           // [n_ot * 16] their inverses
    _Float16 *wp;          // packed halves
    int OC, IC, taps, group, slot, c4, nsteps, n_ot, oc_base, ic_base, ic_total;
};

__global__ __launch_bounds__(256) void train_pack16_rowscale_kernel(const Pack16Args a)
{
    __shared__ float red[4];
    const int oc = blockIdx.x;  // row of THIS weight tensor
    float mx = 0.0f;
    const int n = a.IC * a.taps;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int ic = i / a.taps, t = i - ic * a.taps;
        mx = fmaxf(mx, fabsf(a.w[((size_t)oc * a.ic_total + a.ic_base + ic) * a.taps + t]));
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float rs = 1.0f;
        if (mx > 0.0f && mx < 3.0e38f) {  // row_scale(): the largest magnitude of the row lands in [2^13, 2^14)
            int e = 0;
            (void)frexpf(mx, &e);
            int k = 14 - e;
            k = k > 100 ? 100 : (k < -100 ? -100 : k);
            rs = ldexpf(1.0f, k);
        }
        a.rs[a.oc_base + oc] = rs;
        a.rinv[a.oc_base + oc] = 1.0f / rs;
    }
}

__global__ __launch_bounds__(256) void train_pack16_kernel(const Pack16Args a)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)a.nsteps * a.n_ot * 512;  // (S, ot, lane, j)
    if (i >= total) return;
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
    const long rest = i >> 9;
    const int ot = (int)(rest % a.n_ot), S = (int)(rest / a.n_ot);
    const int row = ot * 16 + (lane & 15), G = 8 * S + 2 * (lane >> 4) + (j >> 2);
    const int oc = row - a.oc_base;
    if (oc < 0 || oc >= a.OC || G >= a.taps * a.c4) return;  // (the buffer starts zeroed; other tensors of a stack own the other rows)
    const int t = G / a.c4, ch = 4 * (G - t * a.c4) + (j & 3);
    const int ic = train_unslot(ch, a.group, a.slot, a.IC);
    float v = 0.0f;
    if (ic >= 0) v = a.rs[row] * a.w[((size_t)oc * a.ic_total + a.ic_base + ic) * a.taps + t];
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    const size_t base = ((size_t)S * a.n_ot + ot) * 2 * 64 * 8;
    a.wp[base + (size_t)lane * 8 + j] = hi;
    a.wp[base + 64 * 8 + (size_t)lane * 8 + j] = lo;
}

// Backward-data form of the same: rows = the convolution's INPUT channels (physical, chunk of <= 128 rows starting at
// row0), K entry (tap, 4 output channels) <- w[oc][ic][taps - 1 - tap]; a stack of up to four weight tensors shares the K
// axis (kper output channels each: the four branch entries of a VortexPooling).
struct Pack16TArgs {
    const float *w[4];     // [OC][ic_total][taps] each
    int n_src, kper;       // K channels [b * kper, b * kper + OC) belong to tensor b
    float *rs, *rinv;      // [rows of the whole layer, padded]
    _Float16 *wp;          // this chunk's packed halves
    int OC, IC, taps, group, slot, c4k, nsteps, n_ot, row0, rows, ic_base, ic_total;
};

__global__ __launch_bounds__(256) void train_pack16t_rowscale_kernel(const Pack16TArgs a)
{
    __shared__ float red[4];
    const int r = blockIdx.x;  // physical input channel
    const int ic = train_unslot(r, a.group, a.slot, a.IC);
    float mx = 0.0f;
    if (ic >= 0)
        for (int b = 0; b < a.n_src; ++b)
            for (int i = threadIdx.x; i < a.OC * a.taps; i += 256) {
                const int oc = i / a.taps, t = i - oc * a.taps;
                mx = fmaxf(mx, fabsf(a.w[b][((size_t)oc * a.ic_total + a.ic_base + ic) * a.taps + t]));
            }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float rs = 1.0f;
        if (mx > 0.0f && mx < 3.0e38f) {
            int e = 0;
            (void)frexpf(mx, &e);
            int k = 14 - e;
            k = k > 100 ? 100 : (k < -100 ? -100 : k);
            rs = ldexpf(1.0f, k);
        }
        a.rs[r] = rs;
        a.rinv[r] = 1.0f / rs;
    }
}

__global__ __launch_bounds__(256) void train_pack16t_kernel(const Pack16TArgs a)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)a.nsteps * a.n_ot * 512;
    if (i >= total) return;
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
    const long rest = i >> 9;
    const int ot = (int)(rest % a.n_ot), S = (int)(rest / a.n_ot);
    const int row = a.row0 + ot * 16 + (lane & 15), G = 8 * S + 2 * (lane >> 4) + (j >> 2);
    float v = 0.0f;
    if (row < a.rows && G < a.taps * a.c4k) {
        const int tap = G / a.c4k, ch = 4 * (G - tap * a.c4k) + (j & 3);
        const int b = ch / a.kper, oc = ch - b * a.kper;
        const int ic = train_unslot(row, a.group, a.slot, a.IC);
        if (b < a.n_src && oc < a.OC && ic >= 0)
            v = a.rs[row] * a.w[b][((size_t)oc * a.ic_total + a.ic_base + ic) * a.taps + (a.taps - 1 - tap)];
    }
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    const size_t base = ((size_t)S * a.n_ot + ot) * 2 * 64 * 8;
    a.wp[base + (size_t)lane * 8 + j] = hi;
    a.wp[base + 64 * 8 + (size_t)lane * 8 + j] = lo;
}

}  // namespace ojf
