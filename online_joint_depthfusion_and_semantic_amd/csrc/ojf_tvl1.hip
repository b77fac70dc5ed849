// TVL1: robust fusion of depth views (Zach, Pock, Bischof: "A globally optimal algorithm for robust TV-L1 range image
// integration", ICCV 2007).  Every voxel keeps a histogram of the truncated distances the views proposed for it, and the fused
// field is the minimiser of  TV(u) + lambda · sum_voxels sum_b h_b |u - l_b|  over the observed voxels - a regularised median
// where every other path into a volume here is a running mean.  The histogram is fused by the voxel-projective sweep of
// ojf_projective.hip / ojf_labels.hip into a record volume of ojf_records.h; the minimiser is found by Chambolle-Pock
// iterations (theta = 1) on the bricks of the box that hold an observed voxel.  The reference's counterpart
// (deps/mesh-fusion/libfusiongpu/fusion_zach_tvl1.cu) sweeps the whole box, sorts 2B+1 values per voxel in shared memory and
// gives the larger share of a vote to the farther bin; this is a definition of its own, restated in numpy by
// tests/tvl1_ref.py, and the GPU tests pin the kernels to it bit for bit.
//
// The histogram volume: a record volume (ojf_records.h) of B value channels, 2 <= B <= OJF_HIST_MAX_BINS: channels 0..B-1 hold
// the running means h_b of the votes, channel B the weight W (0: never observed).  Bin b has its centre at the normalised
// distance l_b = float(2b) / float(B-1) - 1  (-1: -trunc, +1: +trunc).
//
// Normative definition.  All device arithmetic is fp32 with every product, sum, division and square root rounded on its own
// (the build's -ffp-contract=off, correctly rounded division and sqrt); fp16 conversions round to nearest even; min / max are
// IEEE minNum / maxNum (a NaN operand loses).
//
// ojf_fuse_depth_hist, per voxel, for views v = 0..n-1 in that order ("skip": this view leaves the voxel alone):
//     1. steps 1-3 of ojf_fuse_projective exactly (ojf_projview.h) give the pixel's depth d and the voxel's zc;  s = d - zc.
//     2. skip unless s >= -trunc;  with carve == 0 also skip unless s <= trunc.
//     3. t = min(s, trunc) / trunc;  g = (t + 1) · hb with hb = float(B-1) · 0.5;  b0 = min(int(floor(g)), B-2);
//        f = g - float(b0);  vote_b0 = 1 - f, vote_(b0+1) = f, every other vote_b = 0.
//     4. record_fuse (ojf_records.h): w0 = float(W), w1 = w0 + 1;  h_b = half((w0 · float(h_b) + vote_b) / w1), b = 0..B-1;
//        W = half(min(w1, max_weight)).
//
// The solver.  A voxel is observed when float(W) > 0.  Edge a (a = 0, 1, 2 for x, y, z) of voxel x counts when x and x + e_a
// are both observed and inside the box.  Per observed voxel, from its record:
//     P_0 = 0, P_(i+1) = P_i + float(h_i) for i = 0..B-1 (ascending), T = P_B;  W_i = (T - P_i) - P_i for i = 0..B
//     (the sum of the bins at or above i minus the sum of those below, non-increasing in i);
//     start value u0 = canon(clamp(N / T)) with N = the ascending sum of float(h_b) · l_b;
//     clamp(x) = min(max(x, -1), 1), canon(x) = x + 0.0 (a -0 becomes +0: every u written is canonical).
//   The state is u (the caller's, observed voxels only), ub = 2 u^k - u^(k-1) and the dual p (3 components), the last two in
//   the workspace, both in two copies that the iterations alternate between.  A restart sets u = ub = u0 on the observed
//   voxels and p = 0 everywhere, so that the first iteration sees ub = u.
//   One iteration, tl = tau · lambda (rounded to fp32 by the host):
//     dual, per voxel:   q_a = p_a + sigma · (ub(x + e_a) - ub(x)) where edge a counts, else 0;
//                        d = max(1, sqrt((q_0·q_0 + q_1·q_1) + q_2·q_2));  p_a = q_a / d.
//     primal, per observed voxel (m_a = p_a(x - e_a), 0 when x - e_a is outside the box):
//                        v = u + tau · (((p_0 - m_0) + (p_1 - m_1)) + (p_2 - m_2));
//                        c_i = v + tl · W_i;  m = c_B;  for i = 0..B-1: m = max(m, min(c_i, l_i));
//                        u' = canon(clamp(m));  ub = 2·u' - u;  u = u'.
//     m is the median of {l_0..l_(B-1), c_0..c_B} - the l ascend and the c descend, so that the (B+1)-th smallest of the 2B+1
//     values is max_i min(c_i, l_i) with l_B = +inf - which is the prox of lambda·sum_b h_b |u - l_b| at v with step tau.
//   Unobserved voxels are never written and never read into an observed one (their edges do not count).
//
// ojf_tvl1_write, per observed voxel: tsdf = half(trunc · u), weights = the bits of W; the others keep what they hold.
//
// Shape.  Fusion: the label sweep's - one lane owns one voxel for the call and walks the views; a voting view does a
// read-modify-write of the 16- or 32-byte record (record_fuse).  Solver: the workspace arrays (flags, ub, p) are [X,Y,Zp] with
// Zp = Z rounded up to 4, so that a lane's 4 consecutive z voxels are one 16-byte access whatever Z is; the caller's u
// [X,Y,Z] goes as 16-byte accesses when Z is a multiple of 4 and as 4-byte ones otherwise.  The box is cut into bricks of
// kTvX x kTvY x kTvZ = 4 x 8 x 32 voxels (256 lanes of 4 z voxels).  The set-up pass (a block per brick; on a restart, or when
// the caller says the histogram changed) writes per voxel one byte - the three edge bits and "observed" - and per brick
// whether it holds an observed voxel; one block then scans those (block_exclusive_scan) into the list of such bricks.  An
// iteration is ONE launch: blocks take bricks from the list (a grid stride over it - the count stays on the device), stage
// ub of the brick and a one-voxel halo around it in LDS (9.4 KiB), compute the new dual of the brick's voxels and, again, of
// the lower neighbours across its three lower faces - component a only for face a, which is all the divergence needs -
// into LDS (13.6 KiB), and after one barrier do the primal step of their voxels.  Nothing waits for another block: what a
// block reads of other bricks (ub, p) comes from the copies the launch does not write.  The histogram record, the flags and
// the median of an observed voxel stay in registers (loops unrolled to OJF_HIST_MAX_BINS, no per-lane LDS array).
#include "ojf_projview.h"
#include "ojf_records.h"

namespace ojf {

constexpr int kHistBlock = 256;

struct HistArgs {
    uint16_t *vol;
    ProjImages im;
    uint32_t total;
    int Y, Z, n, B, S, carve;
    float trunc, max_weight, hb;
};

struct HistLaunch {
    HistArgs a;
    ProjView v[OJF_HIST_MAX_VIEWS];
};

__global__ __launch_bounds__(kHistBlock) void hist_fuse_kernel(HistLaunch L)
{
    const HistArgs &P = L.a;
    const uint32_t g = blockIdx.x * kHistBlock + threadIdx.x;
    if (g >= P.total) return;
    float xs[1], ys[1], zs[1];
    voxel_indices<1>(g, P.Y, P.Z, xs, ys, zs);
    uint16_t *const rec = P.vol + (size_t)g * (size_t)P.S;
    for (int v = 0; v < P.n; ++v) {
        uint32_t px;
        float s;
        if (!project_depth(L.v[v], P.im, v, xs[0], ys[0], zs[0], px, s)) continue;
        if (!(s >= -P.trunc)) continue;
        if (!P.carve && !(s <= P.trunc)) continue;
        const float t = fminf(s, P.trunc) / P.trunc;
        const float gb = (t + 1.0f) * P.hb;
        const int b0 = min((int)floorf(gb), P.B - 2);
        const float f = gb - (float)b0;
        const float f0 = 1.0f - f;
        record_fuse(rec, P.B, P.max_weight, [&](int k) { return k == b0 ? f0 : (k == b0 + 1 ? f : 0.0f); });
    }
}

// ---- the solver ------------------------------------------------------------------------------------------------------------
constexpr int kTvX = 4, kTvY = 8, kTvZ = 32;     // a brick, in voxels
constexpr int kTvZG = kTvZ / 4;                  // its groups of 4 z voxels
constexpr int kTvBlock = kTvX * kTvY * kTvZG;    // 256 lanes, one group each
constexpr int kTvTileX = kTvX + 2, kTvTileY = kTvY + 2, kTvTileZG = kTvZG + 2;  // the ub tile: one voxel (one group in z) around
constexpr uint32_t kEdgeX = 1, kEdgeY = 2, kEdgeZ = 4, kObserved = 8;           // a voxel's flag byte

struct TvHeader {  // the first 256 bytes of the workspace
    uint32_t count;   // listed bricks
    uint32_t parity;  // which copy of ub / p the next iteration reads
};

struct TvGeom {
    int X, Y, Z, Zp, nbx, nby, nbz;
    uint32_t nbricks;
    size_t Np;  // X·Y·Zp
    size_t off_any, off_offs, off_list, off_flags, off_ub, off_p, bytes;
};

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// false: a box whose padded size the 31-bit indices do not reach
static bool tv_geometry(int X, int Y, int Z, TvGeom &G)
{
    if (!volume_size_ok(X, Y, Z)) return false;
    G.X = X; G.Y = Y; G.Z = Z;
    const int64_t Zp = ((int64_t)Z + 3) & ~(int64_t)3;
    if (!volume_size_ok(X, Y, Zp)) return false;
    G.Zp = (int)Zp;
    G.Np = (size_t)X * Y * Zp;
    G.nbx = (X + kTvX - 1) / kTvX; G.nby = (Y + kTvY - 1) / kTvY; G.nbz = (G.Zp + kTvZ - 1) / kTvZ;
    G.nbricks = (uint32_t)((int64_t)G.nbx * G.nby * G.nbz);
    size_t o = 256;
    G.off_any = o; o = align256(o + 4 * (size_t)G.nbricks);
    G.off_offs = o; o = align256(o + 4 * (size_t)G.nbricks);
    G.off_list = o; o = align256(o + 4 * (size_t)G.nbricks);
    G.off_flags = o; o = align256(o + G.Np);
    G.off_ub = o; o = align256(o + 2 * 4 * G.Np);
    G.off_p = o; o = align256(o + 6 * 4 * G.Np);
    G.bytes = o;
    return true;
}

struct TvArgs {
    const uint16_t *hist;
    float *u;
    TvHeader *hdr;
    uint32_t *any, *offs, *list;
    uint8_t *flags;
    float *ub;  // [2][Np]
    float *p;   // [2][3][Np]
    int X, Y, Z, Zp, nby, nbz, B, S;
    uint32_t nbricks;
    size_t Np;
    int mode, all_bricks, k, vec;  // mode: 1 restart, 2 refresh;  k: the iteration's index in its call;  vec: Z % 4 == 0
    float tau, sigma, tl;
    float l[OJF_HIST_MAX_BINS + 1];
};

struct TvLane {  // where a lane of a brick's block works
    int x, y, z, lx, ly, gz;
    bool in;       // its group lies inside the padded box
    size_t pi;     // the group's index in the [X,Y,Zp] arrays
    size_t di;     // and in the dense [X,Y,Z] ones
};

__device__ __forceinline__ TvLane tv_lane(const TvArgs &A, uint32_t brick)
{
    TvLane L;
    const int t = threadIdx.x;
    L.gz = t & (kTvZG - 1); L.ly = (t / kTvZG) & (kTvY - 1); L.lx = t / (kTvZG * kTvY);
    const int bz = brick % (uint32_t)A.nbz, by = (brick / (uint32_t)A.nbz) % (uint32_t)A.nby, bx = brick / ((uint32_t)A.nbz * (uint32_t)A.nby);
    L.x = bx * kTvX + L.lx; L.y = by * kTvY + L.ly; L.z = bz * kTvZ + 4 * L.gz;
    L.in = L.x < A.X && L.y < A.Y && L.z < A.Zp;
    L.pi = ((size_t)L.x * A.Y + L.y) * A.Zp + L.z;
    L.di = ((size_t)L.x * A.Y + L.y) * A.Z + L.z;
    return L;
}

__device__ __forceinline__ bool tv_observed(const TvArgs &A, int x, int y, int z)
{
    if (x >= A.X || y >= A.Y || z >= A.Z) return false;
    const size_t i = ((size_t)x * A.Y + y) * A.Z + z;
    return h2f(A.hist[i * (size_t)A.S + A.B]) > 0.0f;
}

// the B means of a record as floats, h[b] = 0 for b >= B (registers: every index is a constant after unrolling)
__device__ __forceinline__ void tv_record(const TvArgs &A, size_t voxel, float h[OJF_HIST_MAX_BINS + 1])
{
    const uint16_t *const rec = A.hist + voxel * (size_t)A.S;
    uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    load8(rec, 0, q);
    if (A.S > 8) load8(rec, 1, q + 4);
#pragma unroll
    for (int b = 0; b <= OJF_HIST_MAX_BINS; ++b) h[b] = b < A.B ? h2f((uint16_t)get16(q, b)) : 0.0f;
}

__device__ __forceinline__ float tv_canon_clamp(float x) { return fminf(fmaxf(x, -1.0f), 1.0f) + 0.0f; }

__device__ __forceinline__ float tv_start_value(const TvArgs &A, size_t voxel)
{
    float h[OJF_HIST_MAX_BINS + 1];
    tv_record(A, voxel, h);
    float N = 0.0f, T = 0.0f;
#pragma unroll
    for (int b = 0; b < OJF_HIST_MAX_BINS; ++b)
        if (b < A.B) { N = N + h[b] * A.l[b]; T = T + h[b]; }
    return tv_canon_clamp(N / T);
}

// the primal step of one observed voxel: u' from v
__device__ __forceinline__ float tv_prox(const TvArgs &A, size_t voxel, float v)
{
    float h[OJF_HIST_MAX_BINS + 1], P[OJF_HIST_MAX_BINS + 1];
    tv_record(A, voxel, h);
    float T = 0.0f;
#pragma unroll
    for (int b = 0; b < OJF_HIST_MAX_BINS; ++b) {
        P[b] = T;
        if (b < A.B) T = T + h[b];
    }
    float m = v + A.tl * ((T - T) - T);
#pragma unroll
    for (int i = 0; i < OJF_HIST_MAX_BINS; ++i)
        if (i < A.B) m = fmaxf(m, fminf(v + A.tl * ((T - P[i]) - P[i]), A.l[i]));
    return tv_canon_clamp(m);
}

// the set-up pass: a block per brick
__global__ __launch_bounds__(kTvBlock) void tv_setup_kernel(TvArgs A)
{
    const TvLane L = tv_lane(A, blockIdx.x);
    int seen = 0;
    if (L.in) {
        uint32_t f = 0;
        bool obs[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            obs[e] = tv_observed(A, L.x, L.y, L.z + e);
            if (obs[e]) {
                uint32_t b = kObserved;
                if (tv_observed(A, L.x + 1, L.y, L.z + e)) b |= kEdgeX;
                if (tv_observed(A, L.x, L.y + 1, L.z + e)) b |= kEdgeY;
                if (tv_observed(A, L.x, L.y, L.z + e + 1)) b |= kEdgeZ;
                f |= b << (8 * e);
                seen = 1;
            }
        }
        uint32_t *const fw = reinterpret_cast<uint32_t *>(A.flags + L.pi);
        const uint32_t old = A.mode == 2 ? *fw : 0u;
        *fw = f;
        if (A.mode == 1) {
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int c = 0; c < 6; ++c) *reinterpret_cast<float4 *>(A.p + (size_t)c * A.Np + L.pi) = zero;
        }
        float *const ubc = A.ub + (A.mode == 2 ? (size_t)(A.hdr->parity & 1) * A.Np : 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool fresh = obs[e] && (A.mode == 1 || !((old >> (8 * e)) & kObserved));
            if (fresh) {
                const float u0 = tv_start_value(A, L.di + e);
                A.u[L.di + e] = u0;
                ubc[L.pi + e] = u0;
            } else if (A.mode == 1) {
                ubc[L.pi + e] = 0.0f;
            }
        }
    }
    const int any = __syncthreads_or(seen);
    if (threadIdx.x == 0) A.any[blockIdx.x] = (any || A.all_bricks) ? 1u : 0u;
}

// one block: the list of the bricks that hold an observed voxel
__global__ __launch_bounds__(kScanBlock) void tv_list_kernel(TvArgs A)
{
    const uint32_t total = block_exclusive_scan<uint32_t>(A.any, A.offs, A.nbricks);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < A.nbricks; b += kScanBlock)
        if (A.any[b]) A.list[A.offs[b]] = b;
    if (threadIdx.x == 0) {
        A.hdr->count = total;
        if (A.mode == 1) A.hdr->parity = 0;
    }
}

__global__ void tv_parity_kernel(TvHeader *hdr, uint32_t n) { hdr->parity = (hdr->parity + n) & 1u; }

// the new dual of one voxel: ub at the voxel and at its three upper neighbours, its flag byte, its old p
__device__ __forceinline__ void tv_dual(float u0, float ux, float uy, float uz, uint32_t f, float p0, float p1, float p2, float sigma,
                                        float out[3])
{
    const float q0 = (f & kEdgeX) ? p0 + sigma * (ux - u0) : 0.0f;
    const float q1 = (f & kEdgeY) ? p1 + sigma * (uy - u0) : 0.0f;
    const float q2 = (f & kEdgeZ) ? p2 + sigma * (uz - u0) : 0.0f;
    const float d = fmaxf(1.0f, sqrtf((q0 * q0 + q1 * q1) + q2 * q2));
    out[0] = q0 / d; out[1] = q1 / d; out[2] = q2 / d;
}

__device__ __forceinline__ void f4_to(const float4 &v, float o[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }

__global__ __launch_bounds__(kTvBlock) void tv_iterate_kernel(TvArgs A)
{
    __shared__ __attribute__((aligned(16))) float ub[kTvTileX][kTvTileY][4 * kTvTileZG];
    __shared__ float P0[kTvX + 1][kTvY][kTvZ];  // p_0 of the brick ([1..]) and of the voxels across its lower x face ([0])
    __shared__ float P1[kTvX][kTvY + 1][kTvZ];
    __shared__ float P2[kTvX][kTvY][kTvZ + 1];
    const uint32_t cur = (A.hdr->parity + (uint32_t)A.k) & 1u;
    const float *const ub_cur = A.ub + (size_t)cur * A.Np;
    float *const ub_new = A.ub + (size_t)(cur ^ 1u) * A.Np;
    const float *const p_cur = A.p + (size_t)cur * 3 * A.Np;
    float *const p_new = A.p + (size_t)(cur ^ 1u) * 3 * A.Np;
    const uint32_t count = min(A.hdr->count, A.nbricks);  // (a workspace no set-up pass has seen must not lead past the list)
    const int t = threadIdx.x;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const TvLane L = tv_lane(A, A.list[item]);
        const int x0 = L.x - L.lx, y0 = L.y - L.ly, z0 = L.z - 4 * L.gz;
        // ub of the brick and one voxel (one group in z) around it
        for (int i = t; i < kTvTileX * kTvTileY * kTvTileZG; i += kTvBlock) {
            const int g = i % kTvTileZG, yy = (i / kTvTileZG) % kTvTileY, xx = i / (kTvTileZG * kTvTileY);
            const int x = x0 + xx - 1, y = y0 + yy - 1, z = z0 + 4 * (g - 1);
            float4 v = zero4;
            if (x >= 0 && x < A.X && y >= 0 && y < A.Y && z >= 0 && z < A.Zp)
                v = *reinterpret_cast<const float4 *>(ub_cur + ((size_t)x * A.Y + y) * A.Zp + z);
            *reinterpret_cast<float4 *>(&ub[xx][yy][4 * g]) = v;
        }
        __syncthreads();
        // the dual of the lane's own voxels
        uint32_t f = 0;
        float pn[3][4];
        {
            float po[3][4];
#pragma unroll
            for (int a = 0; a < 3; ++a) f4_to(L.in ? *reinterpret_cast<const float4 *>(p_cur + (size_t)a * A.Np + L.pi) : zero4, po[a]);
            if (L.in) f = *reinterpret_cast<const uint32_t *>(A.flags + L.pi);
            const int xx = L.lx + 1, yy = L.ly + 1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int zz = 4 * (L.gz + 1) + e;
                float o[3];
                tv_dual(ub[xx][yy][zz], ub[xx + 1][yy][zz], ub[xx][yy + 1][zz], ub[xx][yy][zz + 1], f >> (8 * e), po[0][e], po[1][e],
                        po[2][e], A.sigma, o);
                pn[0][e] = o[0]; pn[1][e] = o[1]; pn[2][e] = o[2];
                P0[L.lx + 1][L.ly][4 * L.gz + e] = o[0];
                P1[L.lx][L.ly + 1][4 * L.gz + e] = o[1];
                P2[L.lx][L.ly][4 * L.gz + e + 1] = o[2];
            }
            if (L.in) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    *reinterpret_cast<float4 *>(p_new + (size_t)a * A.Np + L.pi) = make_float4(pn[a][0], pn[a][1], pn[a][2], pn[a][3]);
            }
        }
        // again for the lower neighbours across the three lower faces: component a across face a
        if (t < kTvY * kTvZG + kTvX * kTvZG) {  // the x face (64 groups), the y face (32 groups)
            const bool xface = t < kTvY * kTvZG;
            const int i = xface ? t : t - kTvY * kTvZG;
            const int gz = i & (kTvZG - 1), r = i / kTvZG;  // r: ly on the x face, lx on the y face
            const int x = xface ? x0 - 1 : x0 + r, y = xface ? y0 + r : y0 - 1, z = z0 + 4 * gz;
            const int xx = xface ? 0 : r + 1, yy = xface ? r + 1 : 0;
            const bool in = x >= 0 && x < A.X && y >= 0 && y < A.Y && z < A.Zp;
            const size_t pi = in ? ((size_t)x * A.Y + y) * A.Zp + z : 0;
            float po[3][4];
#pragma unroll
            for (int a = 0; a < 3; ++a) f4_to(in ? *reinterpret_cast<const float4 *>(p_cur + (size_t)a * A.Np + pi) : zero4, po[a]);
            const uint32_t fh = in ? *reinterpret_cast<const uint32_t *>(A.flags + pi) : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int zz = 4 * (gz + 1) + e;
                float o[3];
                tv_dual(ub[xx][yy][zz], ub[xx + 1][yy][zz], ub[xx][yy + 1][zz], ub[xx][yy][zz + 1], fh >> (8 * e), po[0][e], po[1][e],
                        po[2][e], A.sigma, o);
                if (xface) P0[0][r][4 * gz + e] = o[0];
                else P1[r][0][4 * gz + e] = o[1];
            }
        } else if (t < kTvY * kTvZG + kTvX * kTvZG + kTvX * kTvY) {  // the z face (32 voxels)
            const int i = t - (kTvY * kTvZG + kTvX * kTvZG);
            const int ly = i & (kTvY - 1), lx = i / kTvY;
            const int x = x0 + lx, y = y0 + ly, z = z0 - 1;
            float o[3] = {0.0f, 0.0f, 0.0f};
            if (x < A.X && y < A.Y && z >= 0) {
                const size_t pi = ((size_t)x * A.Y + y) * A.Zp + z;
                const int xx = lx + 1, yy = ly + 1, zz = 3;
                tv_dual(ub[xx][yy][zz], ub[xx + 1][yy][zz], ub[xx][yy + 1][zz], ub[xx][yy][zz + 1], A.flags[pi], p_cur[pi],
                        p_cur[A.Np + pi], p_cur[2 * A.Np + pi], A.sigma, o);
            }
            P2[lx][ly][0] = o[2];
        }
        __syncthreads();
        // the primal step of the lane's own voxels
        if (L.in && (f & (kObserved * 0x01010101u))) {
            float uo[4], un[4], ubn[4];
            if (A.vec) {
                f4_to(*reinterpret_cast<const float4 *>(A.u + L.di), uo);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) uo[e] = L.z + e < A.Z ? A.u[L.di + e] : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                un[e] = uo[e];
                ubn[e] = 0.0f;
                if ((f >> (8 * e)) & kObserved) {
                    const int zl = 4 * L.gz + e;
                    const float div = ((pn[0][e] - P0[L.lx][L.ly][zl]) + (pn[1][e] - P1[L.lx][L.ly][zl])) + (pn[2][e] - P2[L.lx][L.ly][zl]);
                    un[e] = tv_prox(A, L.di + e, uo[e] + A.tau * div);
                    ubn[e] = 2.0f * un[e] - uo[e];
                }
            }
            if (A.vec) {
                *reinterpret_cast<float4 *>(A.u + L.di) = make_float4(un[0], un[1], un[2], un[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((f >> (8 * e)) & kObserved) A.u[L.di + e] = un[e];
            }
            *reinterpret_cast<float4 *>(ub_new + L.pi) = make_float4(ubn[0], ubn[1], ubn[2], ubn[3]);
        } else if (L.in) {
            *reinterpret_cast<float4 *>(ub_new + L.pi) = zero4;
        }
        __syncthreads();  // (the next brick overwrites the tiles)
    }
}

struct TvWriteArgs {
    const uint16_t *hist;
    const float *u;
    uint16_t *tsdf, *weights;
    uint32_t total;
    int B, S;
    float trunc;
};

__global__ __launch_bounds__(256) void tv_write_kernel(TvWriteArgs A)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= A.total) return;
    const uint16_t w = A.hist[(size_t)g * (size_t)A.S + A.B];
    if (!(h2f(w) > 0.0f)) return;
    A.tsdf[g] = f2h(A.trunc * A.u[g]);
    A.weights[g] = w;
}

static int check_hist_volume(const char *who, const void *vol, int B)
{
    if (B < 2 || B > OJF_HIST_MAX_BINS) return refuse(who, "n_bins must be in 2..OJF_HIST_MAX_BINS");
    if ((uintptr_t)vol & 15) return refuse(who, "hist_dev must be 16-byte aligned");
    return 0;
}

}  // namespace ojf

OJF_API int ojf_fuse_depth_hist(uint16_t *hist, int n_bins, int X, int Y, int Z, const double *origin, double res, int n,
                                const double *K, const double *E, const float *depth, const uint8_t *mask, int h, int w, float trunc,
                                float max_weight, float near, int carve, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_fuse_depth_hist";
    if (!hist || !origin || !K || !E || !depth) return refuse(who, "null pointer argument");
    if (int rc = check_hist_volume(who, hist, n_bins)) return rc;
    if (!(trunc > 0.0f) || !std::isfinite(trunc)) return refuse(who, "trunc must be > 0 and finite");
    if (carve != 0 && carve != 1) return refuse(who, "carve must be 0 or 1");
    if (int rc = check_projective_views(who, X, Y, Z, origin, res, n, OJF_HIST_MAX_VIEWS, K, E, h, w, max_weight, near)) return rc;
    HistLaunch L;
    HistArgs &A = L.a;
    A.vol = hist;
    fill_proj_images(A.im, depth, mask, h, w, near);
    A.total = (uint32_t)((int64_t)X * Y * Z);
    A.Y = Y; A.Z = Z; A.n = n; A.B = n_bins; A.S = record_size(n_bins); A.carve = carve;
    A.trunc = trunc; A.max_weight = max_weight; A.hb = (float)(n_bins - 1) * 0.5f;
    make_proj_views(K, E, origin, res, n, L.v);
    const uint32_t blocks = (A.total + kHistBlock - 1) / kHistBlock;
    hipLaunchKernelGGL(hist_fuse_kernel, dim3(blocks), dim3(kHistBlock), 0, as_stream(stream), L);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API size_t ojf_tvl1_workspace_bytes(int X, int Y, int Z)
{
    ojf::TvGeom G;
    return ojf::tv_geometry(X, Y, Z, G) ? G.bytes : 0;
}

OJF_API int ojf_tvl1_solve(const uint16_t *hist, int n_bins, int X, int Y, int Z, float lambda, float tau, float sigma, int iterations,
                           int restart, float *u, void *workspace, size_t workspace_bytes, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_tvl1_solve";
    if (!hist || !u || !workspace) return refuse(who, "null pointer argument");
    if (int rc = check_hist_volume(who, hist, n_bins)) return rc;
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    TvGeom G;
    if (!tv_geometry(X, Y, Z, G)) return refuse(who, "volume too large");
    if (!(lambda > 0.0f) || !std::isfinite(lambda)) return refuse(who, "lambda must be > 0 and finite");
    if (!(tau > 0.0f) || !(sigma > 0.0f) || !std::isfinite(tau) || !std::isfinite(sigma)) return refuse(who, "tau and sigma must be > 0 and finite");
    if (!((double)tau * (double)sigma <= 1.0 / 12.0)) return refuse(who, "tau * sigma must be <= 1/12");
    if (iterations < 0) return refuse(who, "negative iterations");
    const int mode = restart & 3, all_bricks = (restart & OJF_TVL1_ALL_BRICKS) ? 1 : 0;
    if (restart < 0 || (restart & ~(3 | OJF_TVL1_ALL_BRICKS)) || mode == 3)
        return refuse(who, "restart must be OJF_TVL1_CONTINUE, _RESTART or _REFRESH, with or without OJF_TVL1_ALL_BRICKS");
    if ((uintptr_t)u & 15) return refuse(who, "u_dev must be 16-byte aligned");
    if ((uintptr_t)workspace & 255) return refuse(who, "workspace_dev must be 256-byte aligned");
    if (workspace_bytes < G.bytes) return refuse(who, "workspace too small");
    TvArgs A;
    char *const ws = static_cast<char *>(workspace);
    A.hist = hist; A.u = u;
    A.hdr = reinterpret_cast<TvHeader *>(ws);
    A.any = reinterpret_cast<uint32_t *>(ws + G.off_any);
    A.offs = reinterpret_cast<uint32_t *>(ws + G.off_offs);
    A.list = reinterpret_cast<uint32_t *>(ws + G.off_list);
    A.flags = reinterpret_cast<uint8_t *>(ws + G.off_flags);
    A.ub = reinterpret_cast<float *>(ws + G.off_ub);
    A.p = reinterpret_cast<float *>(ws + G.off_p);
    A.X = X; A.Y = Y; A.Z = Z; A.Zp = G.Zp; A.nby = G.nby; A.nbz = G.nbz; A.B = n_bins; A.S = record_size(n_bins);
    A.nbricks = G.nbricks; A.Np = G.Np;
    A.mode = mode; A.all_bricks = all_bricks; A.k = 0; A.vec = (Z & 3) == 0;
    A.tau = tau; A.sigma = sigma; A.tl = tau * lambda;
    for (int b = 0; b <= OJF_HIST_MAX_BINS; ++b) A.l[b] = b < n_bins ? (float)(2 * b) / (float)(n_bins - 1) - 1.0f : 0.0f;
    hipStream_t s = as_stream(stream);
    if (mode != 0) {
        hipLaunchKernelGGL(tv_setup_kernel, dim3(G.nbricks), dim3(kTvBlock), 0, s, A);
        hipLaunchKernelGGL(tv_list_kernel, dim3(1), dim3(kScanBlock), 0, s, A);
    }
    const uint32_t grid = G.nbricks < 2048u ? G.nbricks : 2048u;  // 256 CUs x 8 resident blocks, a stride over the list for the rest
    for (int k = 0; k < iterations; ++k) {
        A.k = k;
        hipLaunchKernelGGL(tv_iterate_kernel, dim3(grid), dim3(kTvBlock), 0, s, A);
    }
    if (iterations & 1) hipLaunchKernelGGL(tv_parity_kernel, dim3(1), dim3(1), 0, s, A.hdr, 1u);
    OJF_HIP(hipGetLastError());
    return 0;
}

OJF_API int ojf_tvl1_write(const uint16_t *hist, int n_bins, int X, int Y, int Z, const float *u, float trunc, uint16_t *tsdf,
                           uint16_t *weights, ojf_stream_t stream)
{
    using namespace ojf;
    const char *who = "ojf_tvl1_write";
    if (!hist || !u || !tsdf || !weights) return refuse(who, "null pointer argument");
    if (int rc = check_hist_volume(who, hist, n_bins)) return rc;
    if (int rc = check_volume_size(who, X, Y, Z)) return rc;
    if (!(trunc > 0.0f) || !std::isfinite(trunc)) return refuse(who, "trunc must be > 0 and finite");
    if (((uintptr_t)u & 3) || ((uintptr_t)tsdf & 1) || ((uintptr_t)weights & 1)) return refuse(who, "u_dev, tsdf_dev or weights_dev misaligned");
    TvWriteArgs A;
    A.hist = hist; A.u = u; A.tsdf = tsdf; A.weights = weights;
    A.total = (uint32_t)((int64_t)X * Y * Z);
    A.B = n_bins; A.S = record_size(n_bins); A.trunc = trunc;
    hipLaunchKernelGGL(tv_write_kernel, dim3((A.total + 255) / 256), dim3(256), 0, as_stream(stream), A);
    OJF_HIP(hipGetLastError());
    return 0;
}
