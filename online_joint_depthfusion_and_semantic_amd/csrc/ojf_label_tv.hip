// LABEL TV: the fused class distributions regularised in space - the convex relaxation of the Potts model (Zach, Gallup, Frahm,
// Niethammer: "Fast global labeling for real-time stereo using multiple plane sweeps", VMV 2008; Häne, Zach, Cohen, Angst,
// Pollefeys: "Joint 3D scene reconstruction and class segmentation", CVPR 2013) on the label volume of ojf_labels.hip.  Where
// ojf_label_decide lets every voxel decide alone, here the neighbours have a say: the result is the minimiser, over fields u
// with u(x) in the simplex at every observed voxel, of
//     sum_k sum_x |grad u_k(x)|  -  lambda · sum_x omega(x) · <u(x), P(x)>
// (|.| the Euclidean norm of the three forward differences whose edges count), found by Chambolle-Pock iterations (theta = 1) on
// the bricks of the box that hold an observed voxel.  The reference has no counterpart; this is a definition of its own,
// restated in numpy by tests/label_tv_ref.py, and the GPU tests pin the kernels to it bit for bit.
//
// Normative definition.  All device arithmetic is fp32 with every product, sum, division and square root rounded on its own
// (the build's -ffp-contract=off, correctly rounded division and sqrt); fp16 conversions round to nearest even; min / max are
// IEEE minNum / maxNum (a NaN operand loses).
//
// Input: a label record volume (ojf_records.h) of C classes, 2 <= C <= OJF_LABEL_TV_MAX_CLASSES: channels 0..C-1 hold P_k,
// channel C the weight W.  A voxel is observed when float(W) > 0.  Edge a (a = 0, 1, 2 for x, y, z) of voxel x counts when x and
// x + e_a are both observed and inside the box.  Confidence: omega = min(float(W), w_sat) / w_sat.
//
// The simplex projection Pi(v) of v_0..v_(C-1):
//     for j = 0..C-1:  s_j = the sum, in ascending k from 0.0f, of v_k over the k with v_k >= v_j;  n_j = their count;
//                      theta_j = (s_j - 1) / float(n_j);
//     theta = max_j theta_j;   Pi(v)_k = max(v_k - theta, 0).
//   (theta_j is the threshold the sort-based algorithm would try with the n_j largest values; the right one is the largest.
//   There is no sort, and the result is the same for every order of evaluation of the j.)
//
// The state, per observed voxel: u_k, ub_k and the dual p_(k,a), a = 0..2.  A restart sets u = ub = Pi(float(P_0..P_(C-1))) and
// p = 0 (a record whose P sum to 0 starts at the uniform distribution: theta = -1/C).
// One iteration, tl = tau · lambda (rounded to fp32 by the host):
//     dual, per observed voxel and class:
//         q_a = p_(k,a) + sigma · (ub_k(x + e_a) - ub_k(x)) where edge a counts, else 0;
//         d = max(1, sqrt((q_0·q_0 + q_1·q_1) + q_2·q_2));   p_(k,a) = q_a / d.
//     primal, per observed voxel (m_a = p_(k,a)(x - e_a), 0 when x - e_a is outside the box or unobserved):
//         v_k = (u_k + tau · (((p_(k,0) - m_0) + (p_(k,1) - m_1)) + (p_(k,2) - m_2))) + (tl · omega) · float(P_k);
//         u' = Pi(v);   ub = 2·u' - u;   u = u'.
//   Unobserved voxels are never written and never read into an observed one.
//
// ojf_label_tv_write, per observed voxel: ids = the smallest k with the largest u_k, scores = half(u_k) of that class, and, into
// a second record volume of the same C if one is given, channel k = half(u_k), W copied bit for bit, the padding untouched.
// Every other voxel keeps what it holds.
//
// Shape.  The state is 5·C floats per voxel (600 bytes at C = 30), so it lives on the observed bricks only.  The box is cut
// into the bricks of the TV-L1 solver, kLtvX x kLtvY x kLtvZ = 4 x 8 x 32 voxels (voxel i of a brick: lx = i / 256,
// ly = (i / 32) % 8, lz = i % 32).  The set-up pass (ojf_label_tv_setup: a block per brick, then one block that scans) writes
// per voxel one byte - "observed", the three edge bits and the three bits "edge a of x - e_a counts" - and per brick whether it
// holds an observed voxel, and scans those (block_exclusive_scan) into the brick list and the brick -> slot table (-1: not
// listed); the count of listed bricks stays on the device.  The state arrays u, ub, p_0, p_1, p_2 are slot-major
// [slot][class][1024 voxels]: a wave's accesses to one class of one brick are contiguous.  A neighbour across a brick face is
// found through the slot table, and only when the edge between the two counts - then both are observed and the neighbour's
// brick is listed.  The caller sizes the workspace for `capacity_bricks` slots; when more bricks are listed, every kernel of the
// solve and of the write returns at once and the status word (header and *status_dev) says so.
// An iteration is TWO launches - the dual in place, then the primal in place - so that single copies of ub and p suffice:
// the dual kernel reads ub and writes only the p of its own voxels, the primal kernel reads p and writes only u and ub of its
// own voxels.  Blocks stride over the brick list; nothing waits for another block.  In the primal kernel the C values of a
// voxel and the O(C^2) projection stay in registers (loops unrolled to OJF_LABEL_TV_MAX_CLASSES with compile-time indices;
// channels k >= C hold -inf, which no comparison of the projection selects).
#include "ojf_records.h"

namespace ojf {

constexpr int kLtvX = 4, kLtvY = 8, kLtvZ = 32;          // a brick, in voxels (the TV-L1 solver's)
constexpr int kLtvVoxels = kLtvX * kLtvY * kLtvZ;        // 1024
constexpr int kLtvBlock = kLtvY * kLtvZ;                 // 256 lanes: lane t owns (ly, lz) = (t / 32, t % 32) and walks lx
constexpr int kLtvMaxC = OJF_LABEL_TV_MAX_CLASSES;
constexpr uint32_t kLtvEdgeX = 1, kLtvEdgeY = 2, kLtvEdgeZ = 4, kLtvObserved = 8;  // a voxel's flag byte
constexpr uint32_t kLtvLowX = 16, kLtvLowY = 32, kLtvLowZ = 64;                    // edge a of x - e_a counts
constexpr uint32_t kLtvMagic = 0x4c54560bu;
constexpr int kLtvOk = 0, kLtvOverCapacity = 1, kLtvNoState = 2;                   // the status word

struct LtvHeader {  // the first 256 bytes of the workspace
    uint32_t count;     // listed bricks (the set-up pass)
    int32_t status;     // kLtvOk: the state is that of a solve;  kLtvOverCapacity;  kLtvNoState: set up, never restarted (or a
                        // continue that does not fit the restart's capacity and class count)
    uint32_t capacity;  // slots and classes of the restart that made the state
    int32_t C;
    uint32_t magic;     // kLtvMagic ^ nbricks once the set-up pass has run on this workspace for this box
};

struct LtvGeom {
    int nbx, nby, nbz;
    uint32_t nbricks;
    size_t off_any, off_slot, off_list, off_flags, off_u;  // off_u: the bytes of the set-up pass, and where the state starts
    size_t plane;                                          // floats of one state array: capacity · C · 1024
    size_t bytes;
};

static inline size_t ltv_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// false: a box the 31-bit indices do not reach
static bool ltv_geometry(int X, int Y, int Z, int C, uint32_t capacity, LtvGeom &G)
{
    if (!volume_size_ok(X, Y, Z)) return false;
    G.nbx = (X + kLtvX - 1) / kLtvX; G.nby = (Y + kLtvY - 1) / kLtvY; G.nbz = (Z + kLtvZ - 1) / kLtvZ;
    const int64_t nb = (int64_t)G.nbx * G.nby * G.nbz;
    if (nb * kLtvVoxels > 0x7fffffffLL * 8) return false;  // (a flat box of thin bricks: the flag bytes stay below 2^34)
    G.nbricks = (uint32_t)nb;
    size_t o = 256;
    G.off_any = o; o = ltv_align256(o + 4 * (size_t)G.nbricks);
    G.off_slot = o; o = ltv_align256(o + 4 * (size_t)G.nbricks);
    G.off_list = o; o = ltv_align256(o + 4 * (size_t)G.nbricks);
    G.off_flags = o; o = ltv_align256(o + (size_t)G.nbricks * kLtvVoxels);
    G.off_u = o;
    G.plane = (size_t)capacity * (size_t)C * kLtvVoxels;
    G.bytes = o + 5 * 4 * G.plane;
    return true;
}

struct LtvArgs {
    const uint16_t *vol;
    uint16_t *out;  // the write's second record volume, or NULL
    uint8_t *ids;
    uint16_t *scores;
    LtvHeader *hdr;
    uint32_t *any, *list;
    int32_t *slot;
    uint8_t *flags;
    float *u, *ub, *p0, *p1, *p2;  // [slot][C][1024]
    uint32_t *count_out;
    int32_t *status_out;
    int X, Y, Z, nby, nbz, C, S, mode;
    uint32_t nbricks, capacity;
    float tau, sigma, tl, w_sat;
};

struct LtvVoxel {  // voxel i of brick b
    int x, y, z;
    bool in;   // inside the box
    size_t g;  // its index in the dense [X,Y,Z] volumes
};

__device__ __forceinline__ LtvVoxel ltv_voxel(const LtvArgs &A, uint32_t b, int i)
{
    LtvVoxel V;
    const uint32_t bz = b % (uint32_t)A.nbz, by = (b / (uint32_t)A.nbz) % (uint32_t)A.nby, bx = b / ((uint32_t)A.nbz * (uint32_t)A.nby);
    V.x = (int)bx * kLtvX + (i >> 8); V.y = (int)by * kLtvY + ((i >> 5) & 7); V.z = (int)bz * kLtvZ + (i & 31);
    V.in = V.x < A.X && V.y < A.Y && V.z < A.Z;
    V.g = ((size_t)V.x * A.Y + V.y) * A.Z + V.z;
    return V;
}

__device__ __forceinline__ bool ltv_observed(const LtvArgs &A, int x, int y, int z)
{
    if (x < 0 || y < 0 || z < 0 || x >= A.X || y >= A.Y || z >= A.Z) return false;
    const size_t g = ((size_t)x * A.Y + y) * A.Z + z;
    return h2f(A.vol[g * (size_t)A.S + A.C]) > 0.0f;
}

// Where the state of the neighbour of voxel i of brick b (slot `slot`) along axis AXIS, one step up (UP) or down, starts
// (class 0; class k is k · 1024 floats on).  Only for an edge that counts: the neighbour's brick is listed then.
template <int AXIS, bool UP>
__device__ __forceinline__ size_t ltv_neighbour(const LtvArgs &A, uint32_t b, uint32_t slot, int i)
{
    constexpr int ext = AXIS == 0 ? kLtvX : (AXIS == 1 ? kLtvY : kLtvZ);
    constexpr int ls = AXIS == 0 ? kLtvY * kLtvZ : (AXIS == 1 ? kLtvZ : 1);
    const int l = (i / ls) % ext;
    const uint32_t bs = AXIS == 0 ? (uint32_t)(A.nby * A.nbz) : (AXIS == 1 ? (uint32_t)A.nbz : 1u);
    if (UP ? l + 1 < ext : l > 0) return (size_t)slot * A.C * kLtvVoxels + (UP ? i + ls : i - ls);
    const int32_t ns = A.slot[UP ? b + bs : b - bs];
    return (size_t)ns * A.C * kLtvVoxels + (UP ? i - (ext - 1) * ls : i + (ext - 1) * ls);
}

// P_0..P_(C-1) of a record as floats, `pad` for k >= C (registers: every index is a constant after unrolling).  Whole 16-byte
// chunks are read, so padding halves may pass through a register; none is used.
__device__ __forceinline__ void ltv_record(const uint16_t *rec, int C, float pad, float P[kLtvMaxC])
{
#pragma unroll
    for (int c = 0; c < kLtvMaxC / 8; ++c) {
        uint32_t q[4] = {0, 0, 0, 0};
        if (8 * c < C) load8(rec, c, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) P[8 * c + e] = 8 * c + e < C ? h2f((uint16_t)get16(q, e)) : pad;
    }
}

// Pi(v) in place; v_k = -inf for k >= C on entry (such a k fails every comparison with a finite v_j), 0 on return
__device__ __forceinline__ void ltv_project(float v[kLtvMaxC], int C)
{
    float theta = -INFINITY;
#pragma unroll
    for (int j = 0; j < kLtvMaxC; ++j) {
        if (j < C) {
            float s = 0.0f;
            int n = 0;
#pragma unroll
            for (int k = 0; k < kLtvMaxC; ++k) {
                const bool ge = v[k] >= v[j];
                s = ge ? s + v[k] : s;
                n += ge ? 1 : 0;
            }
            theta = fmaxf(theta, (s - 1.0f) / (float)n);
        }
    }
#pragma unroll
    for (int k = 0; k < kLtvMaxC; ++k) v[k] = fmaxf(v[k] - theta, 0.0f);
}

// ---- the set-up pass ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLtvBlock) void ltv_setup_kernel(LtvArgs A)
{
    const uint32_t b = blockIdx.x;
    int seen = 0;
#pragma unroll
    for (int e = 0; e < kLtvX; ++e) {
        const int i = e * kLtvBlock + (int)threadIdx.x;
        const LtvVoxel V = ltv_voxel(A, b, i);
        uint32_t f = 0;
        if (V.in && ltv_observed(A, V.x, V.y, V.z)) {
            f = kLtvObserved;
            if (ltv_observed(A, V.x + 1, V.y, V.z)) f |= kLtvEdgeX;
            if (ltv_observed(A, V.x, V.y + 1, V.z)) f |= kLtvEdgeY;
            if (ltv_observed(A, V.x, V.y, V.z + 1)) f |= kLtvEdgeZ;
            if (ltv_observed(A, V.x - 1, V.y, V.z)) f |= kLtvLowX;
            if (ltv_observed(A, V.x, V.y - 1, V.z)) f |= kLtvLowY;
            if (ltv_observed(A, V.x, V.y, V.z - 1)) f |= kLtvLowZ;
            seen = 1;
        }
        A.flags[(size_t)b * kLtvVoxels + i] = (uint8_t)f;
    }
    const int any = __syncthreads_or(seen);
    if (threadIdx.x == 0) A.any[b] = any ? 1u : 0u;
}

// one block: the list of the bricks that hold an observed voxel, the slot of every brick, the count
__global__ __launch_bounds__(kScanBlock) void ltv_list_kernel(LtvArgs A)
{
    uint32_t *const offs = reinterpret_cast<uint32_t *>(A.slot);
    const uint32_t total = block_exclusive_scan<uint32_t>(A.any, offs, A.nbricks);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < A.nbricks; b += kScanBlock) {
        if (A.any[b]) A.list[offs[b]] = b;
        else A.slot[b] = -1;
    }
    if (threadIdx.x == 0) {
        A.hdr->count = total;
        A.hdr->status = kLtvNoState;
        A.hdr->capacity = 0;
        A.hdr->C = 0;
        A.hdr->magic = kLtvMagic ^ A.nbricks;
        *A.count_out = total;
    }
}

// ---- the solve ---------------------------------------------------------------------------------------------------------------
// one lane: the status of this solve, into the header (what every other kernel tests) and into *status_dev
__global__ void ltv_begin_kernel(LtvArgs A)
{
    LtvHeader *const h = A.hdr;
    int32_t st;
    if (h->magic != (kLtvMagic ^ A.nbricks)) {
        st = kLtvNoState;  // (no set-up pass has seen this workspace: nothing in it may be used as an index)
        h->count = 0;
    } else if (A.mode == OJF_LABEL_TV_RESTART) {
        st = h->count > A.capacity ? kLtvOverCapacity : kLtvOk;
        h->capacity = A.capacity;
        h->C = A.C;
    } else {
        st = h->status;
        if (st == kLtvOk && (h->capacity != A.capacity || h->C != A.C)) st = kLtvNoState;
    }
    h->status = st;
    *A.status_out = st;
}

// a restart: u = ub = Pi(P) at the observed voxels of the listed bricks, 0 at their other voxels, p = 0
__global__ __launch_bounds__(kLtvBlock) void ltv_restart_kernel(LtvArgs A)
{
    if (A.hdr->status != kLtvOk) return;
    const uint32_t count = A.hdr->count;
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t b = A.list[item];
#pragma unroll 1
        for (int e = 0; e < kLtvX; ++e) {
            const int i = e * kLtvBlock + (int)threadIdx.x;
            const uint32_t f = A.flags[(size_t)b * kLtvVoxels + i];
            const size_t own = (size_t)item * A.C * kLtvVoxels + i;
            float v[kLtvMaxC];
            if (f & kLtvObserved) {
                const LtvVoxel V = ltv_voxel(A, b, i);
                ltv_record(A.vol + V.g * (size_t)A.S, A.C, -INFINITY, v);
                ltv_project(v, A.C);
            } else {
#pragma unroll
                for (int k = 0; k < kLtvMaxC; ++k) v[k] = 0.0f;
            }
#pragma unroll
            for (int k = 0; k < kLtvMaxC; ++k) {
                if (k < A.C) {
                    const size_t o = own + (size_t)k * kLtvVoxels;
                    A.u[o] = v[k]; A.ub[o] = v[k];
                    A.p0[o] = 0.0f; A.p1[o] = 0.0f; A.p2[o] = 0.0f;
                }
            }
        }
    }
}

// the dual step of the observed voxels of the listed bricks, in place: reads ub, writes only the p of its own voxels
__global__ __launch_bounds__(kLtvBlock) void ltv_dual_kernel(LtvArgs A)
{
    if (A.hdr->status != kLtvOk) return;
    const uint32_t count = A.hdr->count;
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t b = A.list[item];
#pragma unroll 1
        for (int e = 0; e < kLtvX; ++e) {
            const int i = e * kLtvBlock + (int)threadIdx.x;
            const uint32_t f = A.flags[(size_t)b * kLtvVoxels + i];
            if (!(f & kLtvObserved)) continue;
            const size_t own = (size_t)item * A.C * kLtvVoxels + i;
            const size_t nx = (f & kLtvEdgeX) ? ltv_neighbour<0, true>(A, b, item, i) : own;
            const size_t ny = (f & kLtvEdgeY) ? ltv_neighbour<1, true>(A, b, item, i) : own;
            const size_t nz = (f & kLtvEdgeZ) ? ltv_neighbour<2, true>(A, b, item, i) : own;
            for (int k = 0; k < A.C; ++k) {
                const size_t ko = (size_t)k * kLtvVoxels, o = own + ko;
                const float u0 = A.ub[o];
                const float q0 = (f & kLtvEdgeX) ? A.p0[o] + A.sigma * (A.ub[nx + ko] - u0) : 0.0f;
                const float q1 = (f & kLtvEdgeY) ? A.p1[o] + A.sigma * (A.ub[ny + ko] - u0) : 0.0f;
                const float q2 = (f & kLtvEdgeZ) ? A.p2[o] + A.sigma * (A.ub[nz + ko] - u0) : 0.0f;
                const float d = fmaxf(1.0f, sqrtf((q0 * q0 + q1 * q1) + q2 * q2));
                A.p0[o] = q0 / d; A.p1[o] = q1 / d; A.p2[o] = q2 / d;
            }
        }
    }
}

// the primal step of the observed voxels of the listed bricks, in place: reads p, writes only u and ub of its own voxels
__global__ __launch_bounds__(kLtvBlock) void ltv_primal_kernel(LtvArgs A)
{
    if (A.hdr->status != kLtvOk) return;
    const uint32_t count = A.hdr->count;
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t b = A.list[item];
#pragma unroll 1
        for (int e = 0; e < kLtvX; ++e) {
            const int i = e * kLtvBlock + (int)threadIdx.x;
            const uint32_t f = A.flags[(size_t)b * kLtvVoxels + i];
            if (!(f & kLtvObserved)) continue;
            const LtvVoxel V = ltv_voxel(A, b, i);
            const uint16_t *const rec = A.vol + V.g * (size_t)A.S;
            const float omega = fminf(h2f(rec[A.C]), A.w_sat) / A.w_sat;
            const float tlo = A.tl * omega;
            float P[kLtvMaxC], v[kLtvMaxC], uo[kLtvMaxC];
            ltv_record(rec, A.C, 0.0f, P);
            const size_t own = (size_t)item * A.C * kLtvVoxels + i;
            const size_t lx = (f & kLtvLowX) ? ltv_neighbour<0, false>(A, b, item, i) : own;
            const size_t ly = (f & kLtvLowY) ? ltv_neighbour<1, false>(A, b, item, i) : own;
            const size_t lz = (f & kLtvLowZ) ? ltv_neighbour<2, false>(A, b, item, i) : own;
#pragma unroll
            for (int k = 0; k < kLtvMaxC; ++k) {
                v[k] = -INFINITY;
                uo[k] = 0.0f;
                if (k < A.C) {
                    const size_t ko = (size_t)k * kLtvVoxels, o = own + ko;
                    uo[k] = A.u[o];
                    const float m0 = (f & kLtvLowX) ? A.p0[lx + ko] : 0.0f;
                    const float m1 = (f & kLtvLowY) ? A.p1[ly + ko] : 0.0f;
                    const float m2 = (f & kLtvLowZ) ? A.p2[lz + ko] : 0.0f;
                    const float div = ((A.p0[o] - m0) + (A.p1[o] - m1)) + (A.p2[o] - m2);
                    v[k] = (uo[k] + A.tau * div) + tlo * P[k];
                }
            }
            ltv_project(v, A.C);
#pragma unroll
            for (int k = 0; k < kLtvMaxC; ++k) {
                if (k < A.C) {
                    const size_t o = own + (size_t)k * kLtvVoxels;
                    A.u[o] = v[k];
                    A.ub[o] = 2.0f * v[k] - uo[k];
                }
            }
        }
    }
}

// ---- the write-back ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLtvBlock) void ltv_write_kernel(LtvArgs A)
{
    // A.capacity: the slots the caller's workspace_bytes hold
    if (A.hdr->magic != (kLtvMagic ^ A.nbricks) || A.hdr->status != kLtvOk || A.hdr->C != A.C || A.hdr->capacity > A.capacity) return;
    const uint32_t count = A.hdr->count;
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t b = A.list[item];
#pragma unroll 1
        for (int e = 0; e < kLtvX; ++e) {
            const int i = e * kLtvBlock + (int)threadIdx.x;
            const uint32_t f = A.flags[(size_t)b * kLtvVoxels + i];
            if (!(f & kLtvObserved)) continue;
            const LtvVoxel V = ltv_voxel(A, b, i);
            const float *const u = A.u + (size_t)item * A.C * kLtvVoxels + i;
            float best = u[0];
            int id = 0;
            for (int k = 1; k < A.C; ++k) {
                const float x = u[(size_t)k * kLtvVoxels];
                if (x > best) { best = x; id = k; }
            }
            A.ids[V.g] = (uint8_t)id;
            A.scores[V.g] = f2h(best);
            if (A.out) {
                uint16_t *const rec = A.out + V.g * (size_t)A.S;
                const uint16_t w = A.vol[V.g * (size_t)A.S + A.C];
                const int full = A.C >> 3;  // chunks that hold class channels only: 16-byte stores
                for (int c = 0; c < full; ++c) {
                    uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int j = 0; j < 8; ++j) set16(q, j, f2h(u[(size_t)(8 * c + j) * kLtvVoxels]));
                    reinterpret_cast<uint4 *>(rec)[c] = make_uint4(q[0], q[1], q[2], q[3]);
                }
                for (int k = 8 * full; k < A.C; ++k) rec[k] = f2h(u[(size_t)k * kLtvVoxels]);
                rec[A.C] = w;
            }
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static int ltv_check_volume(const char *who, const void *vol, int C, int X, int Y, int Z)
{
    if (C < 2 || C > OJF_LABEL_TV_MAX_CLASSES) return refuse(who, "n_classes must be in 2..OJF_LABEL_TV_MAX_CLASSES");
    if ((uintptr_t)vol & 15) return refuse(who, "probs_dev must be 16-byte aligned");
    return check_volume_size(who, X, Y, Z);
}

// the workspace's arrays for `capacity` slots; 0 or a refusal
static int ltv_bind(const char *who, int X, int Y, int Z, int C, uint32_t capacity, const void *workspace, size_t bytes, LtvGeom &G, LtvArgs &A)
{
    if (!ltv_geometry(X, Y, Z, C, capacity, G)) return refuse(who, "volume too large");
    if ((uintptr_t)workspace & 255) return refuse(who, "workspace_dev must be 256-byte aligned");
    if (bytes < G.bytes) return refuse(who, "workspace too small");
    char *const ws = static_cast<char *>(const_cast<void *>(workspace));
    A.hdr = reinterpret_cast<LtvHeader *>(ws);
    A.any = reinterpret_cast<uint32_t *>(ws + G.off_any);
    A.slot = reinterpret_cast<int32_t *>(ws + G.off_slot);
    A.list = reinterpret_cast<uint32_t *>(ws + G.off_list);
    A.flags = reinterpret_cast<uint8_t *>(ws + G.off_flags);
    A.u = reinterpret_cast<float *>(ws + G.off_u);
    A.ub = A.u + G.plane; A.p0 = A.ub + G.plane; A.p1 = A.p0 + G.plane; A.p2 = A.p1 + G.plane;
    A.X = X; A.Y = Y; A.Z = Z; A.nby = G.nby; A.nbz = G.nbz; A.C = C; A.S = record_size(C);
    A.nbricks = G.nbricks; A.capacity = capacity;
    A.out = nullptr; A.ids = nullptr; A.scores = nullptr; A.count_out = nullptr; A.status_out = nullptr;
    A.mode = 0; A.tau = A.sigma = A.tl = A.w_sat = 0.0f;
    return 0;
}

static inline uint32_t ltv_grid(uint32_t bricks) { return bricks < 1u ? 1u : (bricks < 2048u ? bricks : 2048u); }  // 256 CUs x 8 resident blocks

}  // namespace ojf

OJF_API size_t ojf_label_tv_workspace_bytes(int X, int Y, int Z, int n_classes, uint32_t capacity_bricks)
{
    ojf::LtvGeom G;
    if (n_classes < 2 || n_classes > OJF_LABEL_TV_MAX_CLASSES) return 0;
    return ojf::ltv_geometry(X, Y, Z, n_classes, capacity_bricks, G) ? G.bytes : 0;
}

OJF_API int ojf_label_tv_setup(const uint16_t *probs, int n_classes, int X, int Y, int Z, void *workspace, size_t workspace_bytes,
                               uint32_t *count, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_label_tv_setup";
    if (!probs || !workspace || !count) return refuse(who, "null pointer argument");
    if (int rc = ltv_check_volume(who, probs, n_classes, X, Y, Z)) return rc;
    if ((uintptr_t)count & 3) return refuse(who, "count_dev misaligned");
    LtvGeom G;
    LtvArgs A;
    if (int rc = ltv_bind(who, X, Y, Z, n_classes, 0, workspace, workspace_bytes, G, A)) return rc;
    A.vol = probs; A.count_out = count;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ltv_setup_kernel, dim3(G.nbricks), dim3(kLtvBlock), 0, s, A);
    hipLaunchKernelGGL(ltv_list_kernel, dim3(1), dim3(kScanBlock), 0, s, A);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_label_tv_solve(const uint16_t *probs, int n_classes, int X, int Y, int Z, float lambda, float w_sat, float tau, float sigma,
                               int iterations, int mode, uint32_t capacity_bricks, void *workspace, size_t workspace_bytes, int32_t *status,
                               ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_label_tv_solve";
    if (!probs || !workspace || !status) return refuse(who, "null pointer argument");
    if (int rc = ltv_check_volume(who, probs, n_classes, X, Y, Z)) return rc;
    if (!(lambda > 0.0f) || !std::isfinite(lambda)) return refuse(who, "lambda must be > 0 and finite");
    if (!(w_sat > 0.0f) || !std::isfinite(w_sat)) return refuse(who, "w_sat must be > 0 and finite");
    if (!(tau > 0.0f) || !(sigma > 0.0f) || !std::isfinite(tau) || !std::isfinite(sigma)) return refuse(who, "tau and sigma must be > 0 and finite");
    if (!((double)tau * (double)sigma <= 1.0 / 12.0)) return refuse(who, "tau * sigma must be <= 1/12");
    if (iterations < 0) return refuse(who, "negative iterations");
    if (mode != OJF_LABEL_TV_CONTINUE && mode != OJF_LABEL_TV_RESTART) return refuse(who, "mode must be OJF_LABEL_TV_CONTINUE or _RESTART");
    if ((uintptr_t)status & 3) return refuse(who, "status_dev misaligned");
    LtvGeom G;
    LtvArgs A;
    if (int rc = ltv_bind(who, X, Y, Z, n_classes, capacity_bricks, workspace, workspace_bytes, G, A)) return rc;
    A.vol = probs; A.status_out = status; A.mode = mode;
    A.tau = tau; A.sigma = sigma; A.tl = tau * lambda; A.w_sat = w_sat;
    hipStream_t s = as_stream(stream);
    const uint32_t grid = ltv_grid(capacity_bricks < G.nbricks ? capacity_bricks : G.nbricks);
    hipLaunchKernelGGL(ltv_begin_kernel, dim3(1), dim3(1), 0, s, A);
    if (mode == OJF_LABEL_TV_RESTART) hipLaunchKernelGGL(ltv_restart_kernel, dim3(grid), dim3(kLtvBlock), 0, s, A);
    for (int k = 0; k < iterations; ++k) {
        hipLaunchKernelGGL(ltv_dual_kernel, dim3(grid), dim3(kLtvBlock), 0, s, A);
        hipLaunchKernelGGL(ltv_primal_kernel, dim3(grid), dim3(kLtvBlock), 0, s, A);
    }
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_label_tv_write(const uint16_t *probs, int n_classes, int X, int Y, int Z, const void *workspace, size_t workspace_bytes,
                               uint8_t *ids, uint16_t *scores, uint16_t *probs_out, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_label_tv_write";
    if (!probs || !workspace || !ids || !scores) return refuse(who, "null pointer argument");
    if (int rc = ltv_check_volume(who, probs, n_classes, X, Y, Z)) return rc;
    if (((uintptr_t)scores & 1) || ((uintptr_t)probs_out & 15)) return refuse(who, "scores_dev or probs_out_dev misaligned");
    LtvGeom G;
    LtvArgs A;
    if (int rc = ltv_bind(who, X, Y, Z, n_classes, 0, workspace, workspace_bytes, G, A)) return rc;
    // the slots the workspace holds: the kernel refuses a state that was made for more
    const size_t per_slot = 5 * 4 * (size_t)n_classes * kLtvVoxels;
    const size_t fit = (workspace_bytes - G.off_u) / per_slot;
    A.capacity = fit > 0xffffffffu ? 0xffffffffu : (uint32_t)fit;
    A.vol = probs; A.out = probs_out; A.ids = ids; A.scores = scores;
    const uint32_t grid = ltv_grid(A.capacity < G.nbricks ? A.capacity : G.nbricks);
    hipLaunchKernelGGL(ltv_write_kernel, dim3(grid), dim3(kLtvBlock), 0, as_stream(stream), A);
    OJF_HIP(hipGetLastError());
    return 0;
}
