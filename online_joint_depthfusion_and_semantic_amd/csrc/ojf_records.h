// The fp16 record volumes with a weight channel (the class distributions of ojf_labels.hip, the depth histograms of
// ojf_tvl1.hip): fp16 [X,Y,Z,S], voxel-major, 16-byte aligned, S = 8·ceil((C+1)/8) for C value channels; channels 0..C-1 hold
// running means, channel C the weight W (0: nothing fused), the channels behind it are padding that nothing reads or writes.
// One text for the layout and for the running-mean update of a record, so that both volumes round alike.
#pragma once
#include "ojf_blocks.h"

namespace ojf {

// S of a record with C value channels
static inline __host__ __device__ int record_size(int C) { return 8 * ((C + 8) / 8); }

// the running mean of one channel: w0 = float(W), w1 = w0 + 1, p the observation
__device__ __forceinline__ uint16_t record_mean(uint16_t P, float w0, float w1, float p) { return f2h((w0 * h2f(P) + p) / w1); }

// One observation into the record `rec` of C channels, straight in memory: w0 = float(W), w1 = w0 + 1; channel k takes
// half((w0·float(P_k) + value(k)) / w1) for k = 0..C-1, then W = half(min(w1, max_weight)).  The C/8 whole chunks go as 16-byte
// accesses (the 8 observations of a chunk are taken before its means are formed), the C mod 8 channels of the last chunk
// and W as 2-byte accesses, which is what keeps the padding unread.
template <typename Value>
__device__ __forceinline__ void record_fuse(uint16_t *rec, int C, float max_weight, Value value)
{
    const int full = C >> 3;  // chunks that hold value channels only
    const float w0 = h2f(rec[C]);
    const float w1 = w0 + 1.0f;
    for (int c = 0; c < full; ++c) {
        uint4 *const chunk = reinterpret_cast<uint4 *>(rec) + c;
        const uint4 r = *chunk;
        uint32_t q[4] = {r.x, r.y, r.z, r.w};
        float p[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = value(8 * c + e);
#pragma unroll
        for (int e = 0; e < 8; ++e) set16(q, e, record_mean((uint16_t)get16(q, e), w0, w1, p[e]));
        *chunk = make_uint4(q[0], q[1], q[2], q[3]);
    }
    for (int k = 8 * full; k < C; ++k) rec[k] = record_mean(rec[k], w0, w1, value(k));
    rec[C] = f2h(fminf(w1, max_weight));
}

}  // namespace ojf
