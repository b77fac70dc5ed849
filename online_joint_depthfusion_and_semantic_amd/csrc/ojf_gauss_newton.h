// The Gauss-Newton half that ojf_track.hip (frame-to-model ICP) and ojf_register.hip (volume-to-volume registration) share,
// defined once: the 29 fp64 terms of a point, their block sum into one row, and the one-block solve kernel with its 6x6
// Cholesky, Rodrigues update, stats row, status codes and the freeze after a failed step.  The normative text is (b)'s last
// paragraph and (c) of ojf_track.hip's header.  Everything here is `static` or a template: two translation units include it.
#pragma once
#include "ojf_common.h"

#include <math.h>

namespace ojf {

constexpr int kTrackThreads = 256;
constexpr int kTrackPixPerThread = 4;
constexpr int kTrackPixPerBlock = kTrackThreads * kTrackPixPerThread;
constexpr int kTrackTerms = OJF_TRACK_TERMS;
constexpr int kSolveChunk = 64;  // block rows per LDS chunk of the solve (14.8 KB)

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// acc += the 29 terms of one inlier (fp64 products of fp32 values: exact)
__device__ __forceinline__ void add_terms(double acc[kTrackTerms], const float J[6], float res)
{
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) acc[e++] += (double)J[i] * (double)J[j];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += (double)J[i] * (double)res;
    acc[27] += (double)res * (double)res;
    acc[28] += 1.0;
}

// row[0..28] = the block's sums: the lanes of a wave by a shift-down tree (offsets 32, 16, .., 1), the four waves in wave
// order.  Every lane of a block of kTrackThreads calls it.
__device__ __forceinline__ void block_terms_to_row(double acc[kTrackTerms], double *row)
{
#pragma unroll
    for (int e = 0; e < kTrackTerms; ++e) {
        double s = acc[e];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        acc[e] = s;
    }
    __shared__ double part[kTrackThreads / 64][kTrackTerms];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < kTrackTerms; ++e) part[wave][e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < kTrackTerms) {
        double s = 0.0;
        for (int wv = 0; wv < kTrackThreads / 64; ++wv) s += part[wv][threadIdx.x];
        row[threadIdx.x] = s;
    }
}

struct SolveArgs {
    const double *rows;
    int nblocks;
    double *pose;
    int *status;
    double *stats;   // row `iter` of [n_iter, 4]
    double *sums;    // [29] or NULL
    int iter;
    double min_count;
    double init[12];
};

__device__ static bool solve6(const double A[6][6], const double b[6], double x[6])
{
    double dmax = A[0][0];
    for (int j = 1; j < 6; ++j) dmax = fmax(dmax, A[j][j]);
    const double thr = 1e-6 * dmax;
    double L[6][6] = {};
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d > thr)) return false;
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

static __global__ __launch_bounds__(kTrackThreads) void track_solve_kernel(SolveArgs S)
{
    // the rows arrive in LDS a chunk at a time with independent loads; lane e then adds its column in block order (a
    // chain of dependent global loads would cost ~0.2 us per block).  The next chunk's loads are in flight meanwhile: a
    // registration has thousands of rows, and one exposed round trip to memory per chunk was most of the kernel's time.
    __shared__ double chunk[kSolveChunk * kTrackTerms];
    __shared__ double sum[kTrackTerms];
    const int frozen = S.status[0];
    if (frozen) {
        if (threadIdx.x == 0) {
            double *st = S.stats + 4 * (size_t)S.iter;
            st[0] = st[1] = st[2] = st[3] = 0.0;
        }
        return;
    }
    constexpr int kMine = (kSolveChunk * kTrackTerms + kTrackThreads - 1) / kTrackThreads;
    const size_t total = (size_t)S.nblocks * kTrackTerms;
    double next[kMine];
#pragma unroll
    for (int k = 0; k < kMine; ++k) {
        const size_t i = (size_t)k * kTrackThreads + threadIdx.x;
        next[k] = i < total && k * kTrackThreads + (int)threadIdx.x < kSolveChunk * kTrackTerms ? S.rows[i] : 0.0;
    }
    double acc = 0.0;
    for (int b0 = 0; b0 < S.nblocks; b0 += kSolveChunk) {
        const int nb = S.nblocks - b0 < kSolveChunk ? S.nblocks - b0 : kSolveChunk;
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int i = k * kTrackThreads + (int)threadIdx.x;
            if (i < kSolveChunk * kTrackTerms) chunk[i] = next[k];
        }
        __syncthreads();
        const size_t ahead = (size_t)(b0 + kSolveChunk) * kTrackTerms;
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            const int i = k * kTrackThreads + (int)threadIdx.x;
            next[k] = i < kSolveChunk * kTrackTerms && ahead + i < total ? S.rows[ahead + i] : 0.0;
        }
        if (threadIdx.x < kTrackTerms)
            for (int b = 0; b < nb; ++b) acc += chunk[b * kTrackTerms + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < kTrackTerms) {
        sum[threadIdx.x] = acc;
        if (S.sums) S.sums[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double *st = S.stats + 4 * (size_t)S.iter;
    const double cnt = sum[28];
    st[0] = cnt;
    st[1] = cnt > 0.0 ? sum[27] / cnt : 0.0;
    st[2] = st[3] = 0.0;
    int code = 0;
    double x[6];
    if (cnt < S.min_count) {
        code = 1;
    } else {
        double A[6][6], b[6];
        int e = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = sum[e++];
        for (int i = 0; i < 6; ++i) b[i] = -sum[21 + i];
        if (!solve6(A, b, x)) code = 2;
        else
            for (int i = 0; i < 6; ++i)
                if (!isfinite(x[i])) code = 3;
    }
    if (code) {
        S.status[0] = code;
        S.status[1] = S.iter;
        for (int i = 0; i < 12; ++i) S.pose[i] = S.init[i];
        return;
    }
    const double w[3] = {x[0], x[1], x[2]}, tau[3] = {x[3], x[4], x[5]};
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double Ri[3][3];
    if (th < 1e-12) {
        Ri[0][0] = 1.0; Ri[0][1] = -w[2]; Ri[0][2] = w[1];
        Ri[1][0] = w[2]; Ri[1][1] = 1.0; Ri[1][2] = -w[0];
        Ri[2][0] = -w[1]; Ri[2][1] = w[0]; Ri[2][2] = 1.0;
    } else {
        const double k[3] = {w[0] / th, w[1] / th, w[2] / th};
        const double s = sin(th), c = 1.0 - cos(th);
        const double Kx[3][3] = {{0.0, -k[2], k[1]}, {k[2], 0.0, -k[0]}, {-k[1], k[0], 0.0}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double dl = i == j ? 1.0 : 0.0;
                Ri[i][j] = (dl + s * Kx[i][j]) + c * (k[i] * k[j] - dl);
            }
    }
    double P[12];
    for (int i = 0; i < 12; ++i) P[i] = S.pose[i];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) S.pose[4 * i + j] = Ri[i][0] * P[j] + Ri[i][1] * P[4 + j] + Ri[i][2] * P[8 + j];
        S.pose[4 * i + 3] = (Ri[i][0] * P[3] + Ri[i][1] * P[7] + Ri[i][2] * P[11]) + tau[i];
    }
    st[2] = th;
    st[3] = sqrt(tau[0] * tau[0] + tau[1] * tau[1] + tau[2] * tau[2]);
}

static inline void fill_solve(SolveArgs &S, const double *rows, int nblocks, double *pose, int *status, double *stats,
                              double *sums, int iter, double min_count, const double *init)
{
    S.rows = rows; S.nblocks = nblocks; S.pose = pose; S.status = status; S.stats = stats; S.sums = sums;
    S.iter = iter; S.min_count = min_count;
    for (int i = 0; i < 12; ++i) S.init[i] = init[i];
}

static inline int launch_solve(const SolveArgs &S, hipStream_t s)
{
    hipLaunchKernelGGL(track_solve_kernel, dim3(1), dim3(kTrackThreads), 0, s, S);
    OJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace ojf
