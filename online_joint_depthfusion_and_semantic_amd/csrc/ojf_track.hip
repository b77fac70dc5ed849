// TRACK: frame-to-model camera tracking (KinectFusion-style projective point-to-plane ICP) against ray casts of the fused
// volume (ojf_render).  Own definition (the reference takes every pose from its dataset); tests/track_ref.py restates it in
// numpy, and the GPU tests pin the pyramid, J, r and the reason codes to it bit for bit and the fp64 sums / solve to 1e-12.
//
// Normative definition.  fp32 arithmetic has every product, sum, division and sqrt rounded on its own (the build's
// -ffp-contract=off, correctly rounded division and sqrt); "a + b + c" means (a + b) + c.  fp64 likewise.
//   Levels l = 0..L-1 (1 <= L <= OJF_TRACK_MAX_LEVELS), level l is (h>>l) x (w>>l).  Host, fp64: fx_l = fx/2^l,
//   fy_l = fy/2^l, cx_l = (cx + 0.5)/2^l - 0.5, cy_l likewise; the kernels use fp32(fx_l) .. fp32(cy_l).  Ki = Kinv_l f32[9]
//   as the caller forms it (render.py: fp32(K_l).inverse()), so live pixels and the model's ray casts share one frame.
//   dc(r, c)_i = Ki[3i]·c + Ki[3i+1]·r + Ki[3i+2]                                   (render's ray form)
// (a) Pyramid.  D_0 = depth where isfinite(depth) && depth > 0 && (no mask || mask != 0), else 0.  D_{l+1}(r, c) from the
//   block b = (D_l(2r,2c), D_l(2r,2c+1), D_l(2r+1,2c), D_l(2r+1,2c+1)): d_min = fminf over the non-zero entries; the value
//   is 0 when no entry is non-zero, else S / (float)n where S sums (in block order, from 0) the n non-zero entries with
//   (d - d_min) <= delta.
// (b) Associate, pixel (r, c) of level l, D = D_l(r, c):
//   v = D·dc(r, c) (per component).  reason 1 when D == 0.
//   a = V(r+1, c) - v, b = V(r, c+1) - v (V = D_l·dc at that pixel); x = a × b = (a1·b2 - a2·b1, a2·b0 - a0·b2,
//   a0·b1 - a1·b0); xx = x0·x0 + x1·x1 + x2·x2; n_c = x / sqrt(xx).  reason 2 on the last row or column, when either
//   neighbour has D_l == 0, or when xx == 0 (or is not finite).  n_c points to the camera (free space).
//   Pose P f64[12] in device memory, rounded once to fp32 (R, t).  p_i = R[i0]·v0 + R[i1]·v1 + R[i2]·v2 + t_i;
//   nw_i = R[i0]·n0 + R[i1]·n1 + R[i2]·n2.
//   Reference camera (Rr, tr) fp32 by value (host: fp32 of E_ref): e = p - tr; q_i = Rr[0i]·e0 + Rr[1i]·e1 + Rr[2i]·e2.
//   reason 3 unless q2 > 0.  ux = fx_l·(q0/q2) + cx_l, uy = fy_l·(q1/q2) + cy_l; col = floor(ux + 0.5),
//   row = floor(uy + 0.5); reason 4 unless 0 <= col < w_l and 0 <= row < h_l (compared as fp32).
//   d_m = model depth at (row, col); reason 5 when d_m == 0.  mc = d_m·dc(row, col);
//   m_i = Rr[i0]·mc0 + Rr[i1]·mc1 + Rr[i2]·mc2 + tr_i.  g = p - m; reason 6 when g0·g0 + g1·g1 + g2·g2 > dist2.
//   n_m = model normal at (row, col); reason 7 when nw0·nm0 + nw1·nm1 + nw2·nm2 < cos_thr (host: dist2 =
//   fp32(dist_thresh^2), cos_thr = fp32(cos(angle_thresh·pi/180)), both from fp64).  Otherwise reason 0, an inlier:
//   r = nm0·g0 + nm1·g1 + nm2·g2;  J = (p × n_m, n_m) with p × n = (p1·n2 - p2·n1, p2·n0 - p0·n2, p0·n1 - p1·n0)
//   (the left update p' = p + w × p + tau, xi = (w, tau)).
//   Terms (fp64 products of fp32 values: exact): e = 0..20 the upper triangle J_i·J_j (i <= j, row-major), 21..26 J_i·r,
//   27 r·r, 28 the count (1).  Block sums: every lane adds its pixels' terms in pixel order from 0; the wave's lanes are
//   combined by a shift-down tree (offsets 32, 16, .., 1), the block's four waves in wave order.  One row of 29 per block.
// (c) Solve, one block: s_e = sum of the rows in block order from 0.  A_ij = A_ji = s_idx(i,j), b_i = -s_{21+i}.
//   Fails (status code 1) when s_28 < min_count = min_inlier_fraction·h_l·w_l (fp64, host).  Cholesky: for j = 0..5:
//   d = A_jj - L_j0·L_j0 - .. - L_j(j-1)·L_j(j-1); fails (code 2) unless d > 1e-6·max_j A_jj (fmax in j order);
//   L_jj = sqrt(d); for i > j: L_ij = (A_ij - L_i0·L_j0 - .. - L_i(j-1)·L_j(j-1)) / L_jj.  y_i = (b_i - L_i0·y_0 - ..) / L_ii
//   (i ascending), xi_i = (y_i - L_(i+1)i·xi_(i+1) - .. - L_5i·xi_5) / L_ii (i descending).  Fails (code 3) unless
//   every xi_i is finite.  w = xi_0..2, tau = xi_3..5; th = sqrt(w0·w0 + w1·w1 + w2·w2).  th < 1e-12: R_inc = I + [w]x;
//   else k = w / th, s = sin(th), c = 1 - cos(th), R_inc_ij = (delta_ij + s·[k]x_ij) + c·(k_i·k_j - delta_ij).
//   P <- [R_inc·R | R_inc·t + tau] with (A·B)_ij = A_i0·B_0j + A_i1·B_1j + A_i2·B_2j.  Stats row (s_28, s_27 / s_28 (0 when
//   s_28 == 0), th, sqrt(tau·tau)).  A failed step writes (s_28, s_27 / s_28, 0, 0), status {code, iteration}, and
//   resets P to E_init; every later association and solve of the call is skipped (its stats row is 0).
// Launches: one pyramid (which also writes P = E_init and the status {0, -1}), then per level from L-1 down to 0 and per
// iteration one associate and one solve: 1 + 2·sum(iterations).  Kernel boundaries order the iterations; the host never
// waits.  No atomics, no inline assembly; every output is written once: the same bits on every run.
// The terms, the block sums and the solve kernel of (b) and (c) are in ojf_gauss_newton.h, which ojf_register.hip shares.
#include "ojf_gauss_newton.h"

namespace ojf {

struct PyramidArgs {
    const float *depth;
    const uint8_t *mask;
    float *pyr;          // levels back to back
    int h, w, levels;
    int off[OJF_TRACK_MAX_LEVELS + 1];  // pixel offset of level l (off[levels] = total)
    float delta;
    double *pose;        // NULL: no initialisation
    int *status;
    double init[12];
};

__device__ __forceinline__ float level0(const PyramidArgs &A, int r, int c)
{
    const size_t i = (size_t)r * A.w + c;
    const float d = A.depth[i];
    const bool ok = isfinite(d) && d > 0.0f && (!A.mask || A.mask[i] != 0);
    return ok ? d : 0.0f;
}

__device__ __forceinline__ float block_value(const float v[4], float delta)
{
    float dmin = INFINITY;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v[k] != 0.0f) {
            dmin = fminf(dmin, v[k]);
            any = true;
        }
    }
    if (!any) return 0.0f;
    float s = 0.0f;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v[k] != 0.0f && (v[k] - dmin) <= delta) {
            s = s + v[k];
            ++n;
        }
    }
    return s / (float)n;
}

template <int LV>
__device__ float pyr_value(const PyramidArgs &A, int r, int c)
{
    if constexpr (LV == 0) {
        return level0(A, r, c);
    } else {
        const float v[4] = {pyr_value<LV - 1>(A, 2 * r, 2 * c), pyr_value<LV - 1>(A, 2 * r, 2 * c + 1),
                            pyr_value<LV - 1>(A, 2 * r + 1, 2 * c), pyr_value<LV - 1>(A, 2 * r + 1, 2 * c + 1)};
        return block_value(v, A.delta);
    }
}

__global__ __launch_bounds__(kTrackThreads) void track_pyramid_kernel(PyramidArgs A)
{
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g == 0 && A.pose) {
        for (int i = 0; i < 12; ++i) A.pose[i] = A.init[i];
        A.status[0] = 0;
        A.status[1] = -1;
    }
    if (g >= A.off[A.levels]) return;
    int l = 0;
    while (l + 1 < A.levels && g >= A.off[l + 1]) ++l;
    const int wl = A.w >> l;
    const int pix = g - A.off[l];
    const int r = pix / wl, c = pix % wl;
    float v;
    switch (l) {
    case 0: v = pyr_value<0>(A, r, c); break;
    case 1: v = pyr_value<1>(A, r, c); break;
    case 2: v = pyr_value<2>(A, r, c); break;
    default: v = pyr_value<3>(A, r, c); break;
    }
    A.pyr[g] = v;
}

struct AssocArgs {
    const float *D;           // level depth [h_l, w_l]
    const float *mdepth;      // model depth [h_l, w_l]
    const float *mnormal;     // model normals [h_l, w_l, 3]
    const double *pose;       // current pose f64[12]
    const int *status;
    double *rows;             // [blocks, 29]
    float *jr;                // [h_l*w_l, 7] or NULL
    uint8_t *reason;          // [h_l*w_l] or NULL
    int h, w, npix;
    float Ki[9];
    float fx, fy, cx, cy;
    float Rr[9], tr[3];
    float dist2, cos_thr;
};

__device__ __forceinline__ void ray_dc(const float Ki[9], int r, int c, float dc[3])
{
    const float cf = (float)c, rf = (float)r;
#pragma unroll
    for (int i = 0; i < 3; ++i) dc[i] = Ki[3 * i] * cf + Ki[3 * i + 1] * rf + Ki[3 * i + 2];
}

__device__ __forceinline__ void vertex(const AssocArgs &A, int r, int c, float D, float V[3])
{
    float dc[3];
    ray_dc(A.Ki, r, c, dc);
#pragma unroll
    for (int i = 0; i < 3; ++i) V[i] = D * dc[i];
}

// reason code of pixel `pix`; for an inlier also J[6] and the residual
__device__ int associate_pixel(const AssocArgs &A, const float R[9], const float t[3], int pix, float J[6], float &res)
{
    const int r = pix / A.w, c = pix % A.w;
    const float D = A.D[pix];
    if (D == 0.0f) return 1;
    if (r + 1 >= A.h || c + 1 >= A.w) return 2;
    const float Dd = A.D[pix + A.w], Dr = A.D[pix + 1];
    if (Dd == 0.0f || Dr == 0.0f) return 2;
    float v[3], vd[3], vr[3];
    vertex(A, r, c, D, v);
    vertex(A, r + 1, c, Dd, vd);
    vertex(A, r, c + 1, Dr, vr);
    float a[3], b[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i] = vd[i] - v[i];
        b[i] = vr[i] - v[i];
    }
    const float x[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const float xx = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (!(xx > 0.0f) || !isfinite(xx)) return 2;
    const float xl = sqrtf(xx);
    const float n[3] = {x[0] / xl, x[1] / xl, x[2] / xl};
    float p[3], nw[3], e[3], q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2] + t[i];
        nw[i] = R[3 * i] * n[0] + R[3 * i + 1] * n[1] + R[3 * i + 2] * n[2];
        e[i] = p[i] - A.tr[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = A.Rr[i] * e[0] + A.Rr[3 + i] * e[1] + A.Rr[6 + i] * e[2];
    if (!(q[2] > 0.0f)) return 3;
    const float ux = A.fx * (q[0] / q[2]) + A.cx, uy = A.fy * (q[1] / q[2]) + A.cy;
    const float fc = floorf(ux + 0.5f), fr = floorf(uy + 0.5f);
    if (!(fc >= 0.0f && fc < (float)A.w && fr >= 0.0f && fr < (float)A.h)) return 4;
    const int mc_ = (int)fc, mr = (int)fr;
    const int mp = mr * A.w + mc_;
    const float dm = A.mdepth[mp];
    if (dm == 0.0f) return 5;
    float mv[3], m[3], g[3];
    vertex(A, mr, mc_, dm, mv);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        m[i] = A.Rr[3 * i] * mv[0] + A.Rr[3 * i + 1] * mv[1] + A.Rr[3 * i + 2] * mv[2] + A.tr[i];
        g[i] = p[i] - m[i];
    }
    if (g[0] * g[0] + g[1] * g[1] + g[2] * g[2] > A.dist2) return 6;
    const float nm[3] = {A.mnormal[3 * (size_t)mp], A.mnormal[3 * (size_t)mp + 1], A.mnormal[3 * (size_t)mp + 2]};
    if (nw[0] * nm[0] + nw[1] * nm[1] + nw[2] * nm[2] < A.cos_thr) return 7;
    res = nm[0] * g[0] + nm[1] * g[1] + nm[2] * g[2];
    J[0] = p[1] * nm[2] - p[2] * nm[1];
    J[1] = p[2] * nm[0] - p[0] * nm[2];
    J[2] = p[0] * nm[1] - p[1] * nm[0];
    J[3] = nm[0];
    J[4] = nm[1];
    J[5] = nm[2];
    return 0;
}

__global__ __launch_bounds__(kTrackThreads) void track_associate_kernel(AssocArgs A)
{
    if (A.status[0] != 0) return;  // a failed step froze the pose: nothing more to do (uniform over the grid)
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) R[3 * i + k] = (float)A.pose[4 * i + k];
        t[i] = (float)A.pose[4 * i + 3];
    }
    double acc[kTrackTerms];
#pragma unroll
    for (int e = 0; e < kTrackTerms; ++e) acc[e] = 0.0;
    for (int k = 0; k < kTrackPixPerThread; ++k) {
        const int pix = (int)blockIdx.x * kTrackPixPerBlock + k * kTrackThreads + (int)threadIdx.x;
        if (pix >= A.npix) break;
        float J[6] = {0, 0, 0, 0, 0, 0}, res = 0.0f;
        const int why = associate_pixel(A, R, t, pix, J, res);
        if (A.reason) A.reason[pix] = (uint8_t)why;
        if (A.jr) {
#pragma unroll
            for (int i = 0; i < 6; ++i) A.jr[7 * (size_t)pix + i] = why ? 0.0f : J[i];
            A.jr[7 * (size_t)pix + 6] = why ? 0.0f : res;
        }
        if (why) continue;
        add_terms(acc, J, res);
    }
    block_terms_to_row(acc, A.rows + (size_t)blockIdx.x * kTrackTerms);
}

static int level_blocks(int h, int w, int l) { return (((h >> l) * (w >> l)) + kTrackPixPerBlock - 1) / kTrackPixPerBlock; }

static size_t pyramid_bytes(int h, int w, int levels)
{
    size_t n = 0;
    for (int l = 0; l < levels; ++l) n += (size_t)(h >> l) * (size_t)(w >> l);
    return align256(n * sizeof(float));
}

static size_t workspace_bytes(int h, int w, int levels)
{
    return pyramid_bytes(h, w, levels) + align256((size_t)level_blocks(h, w, 0) * kTrackTerms * sizeof(double)) + 256;
}

static int check_shape(const char *who, int h, int w, int levels)
{
    if (levels < 1 || levels > OJF_TRACK_MAX_LEVELS) return fail(std::string(who) + ": levels must be 1..OJF_TRACK_MAX_LEVELS");
    if (h <= 0 || w <= 0 || (int64_t)h * w > 0x3fffffffLL) return fail(std::string(who) + ": bad image size");
    if ((h >> (levels - 1)) < 8 || (w >> (levels - 1)) < 8)
        return fail(std::string(who) + ": every level must be at least 8 x 8 pixels");
    return 0;
}

static int check_thresholds(const char *who, double dist, double angle, double delta, double frac)
{
    if (!(dist > 0.0) || !isfinite(dist) || !(angle > 0.0) || !(angle <= 180.0) || !(delta >= 0.0) || !isfinite(delta) ||
        !(frac >= 0.0) || !(frac <= 1.0))
        return fail(std::string(who) + ": thresholds out of range");
    return 0;
}

static void fill_pyramid(PyramidArgs &P, const float *depth, const uint8_t *mask, void *ws, int h, int w, int levels,
                         double delta, double *pose, int *status, const double *init)
{
    P.depth = depth; P.mask = mask; P.pyr = (float *)ws;
    P.h = h; P.w = w; P.levels = levels;
    int off = 0;
    for (int l = 0; l <= OJF_TRACK_MAX_LEVELS; ++l) {
        P.off[l] = off;
        if (l < levels) off += (h >> l) * (w >> l);
    }
    P.delta = (float)delta;
    P.pose = pose; P.status = status;
    for (int i = 0; i < 12; ++i) P.init[i] = init[i];
}

static void fill_assoc(AssocArgs &A, const PyramidArgs &P, int l, const double *K, const float *Ki,
                       const float *mdepth, const float *mnormal, const double *Eref, double dist, double angle,
                       double *pose, const int *status, double *rows)
{
    A.D = P.pyr + P.off[l];
    A.mdepth = mdepth; A.mnormal = mnormal; A.pose = pose; A.status = status; A.rows = rows;
    A.jr = nullptr; A.reason = nullptr;
    A.h = P.h >> l; A.w = P.w >> l; A.npix = A.h * A.w;
    for (int i = 0; i < 9; ++i) A.Ki[i] = Ki[i];
    const double s = (double)(1 << l);
    A.fx = (float)(K[0] / s);
    A.fy = (float)(K[4] / s);
    A.cx = (float)((K[2] + 0.5) / s - 0.5);
    A.cy = (float)((K[5] + 0.5) / s - 0.5);
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) A.Rr[3 * i + k] = (float)Eref[4 * i + k];
        A.tr[i] = (float)Eref[4 * i + 3];
    }
    A.dist2 = (float)(dist * dist);
    A.cos_thr = (float)cos(angle * M_PI / 180.0);
}

static int launch_pyramid(const PyramidArgs &P, hipStream_t s)
{
    const int total = P.off[P.levels];
    hipLaunchKernelGGL(track_pyramid_kernel, dim3((total + kTrackThreads - 1) / kTrackThreads), dim3(kTrackThreads), 0, s, P);
    OJF_HIP(hipGetLastError());
    return 0;
}

static int launch_step(const AssocArgs &A, const SolveArgs &S, hipStream_t s)
{
    hipLaunchKernelGGL(track_associate_kernel, dim3(S.nblocks), dim3(kTrackThreads), 0, s, A);
    OJF_HIP(hipGetLastError());
    return launch_solve(S, s);
}

}  // namespace ojf

OJF_API size_t ojf_track_workspace_bytes(int h, int w, int levels)
{
    using namespace ojf;
    if (levels < 1 || levels > OJF_TRACK_MAX_LEVELS || h <= 0 || w <= 0 || (int64_t)h * w > 0x3fffffffLL) return 0;
    return workspace_bytes(h, w, levels);
}

OJF_API int ojf_track(const float *depth_dev, const uint8_t *mask_dev, int h, int w, int levels, const double *K_host,
                      const float *Kinv_host, const float *const *model_depth_host, const float *const *model_normals_host,
                      const double *E_ref_host, const double *E_init_host, const int *iterations_host, double dist_thresh,
                      double angle_thresh_deg, double pyramid_delta, double min_inlier_fraction, void *workspace_dev,
                      size_t workspace_bytes_, double *pose_dev, double *stats_dev, int *status_dev, ojf_stream_t stream)
{
    using namespace ojf;
    if (!depth_dev || !K_host || !Kinv_host || !model_depth_host || !model_normals_host || !E_ref_host || !E_init_host ||
        !iterations_host || !workspace_dev || !pose_dev || !stats_dev || !status_dev)
        return fail("ojf_track: null pointer argument");
    if (int rc = check_shape("ojf_track", h, w, levels)) return rc;
    int total = 0;
    for (int l = 0; l < levels; ++l) {
        if (!model_depth_host[l] || !model_normals_host[l]) return fail("ojf_track: null pointer argument (model maps)");
        if (iterations_host[l] < 0) return fail("ojf_track: negative iteration count");
        total += iterations_host[l];
        if (total > OJF_TRACK_MAX_ITERATIONS) return fail("ojf_track: more than OJF_TRACK_MAX_ITERATIONS iterations");
    }
    if (int rc = check_thresholds("ojf_track", dist_thresh, angle_thresh_deg, pyramid_delta, min_inlier_fraction)) return rc;
    if (workspace_bytes_ < workspace_bytes(h, w, levels)) return fail("ojf_track: workspace too small");
    const hipStream_t s = as_stream(stream);
    PyramidArgs P;
    fill_pyramid(P, depth_dev, mask_dev, workspace_dev, h, w, levels, pyramid_delta, pose_dev, status_dev, E_init_host);
    double *rows = (double *)((char *)workspace_dev + pyramid_bytes(h, w, levels));
    if (int rc = launch_pyramid(P, s)) return rc;
    int iter = 0;
    for (int l = levels - 1; l >= 0; --l) {
        AssocArgs A;
        fill_assoc(A, P, l, K_host, Kinv_host + 9 * l, model_depth_host[l], model_normals_host[l], E_ref_host,
                   dist_thresh, angle_thresh_deg, pose_dev, status_dev, rows);
        SolveArgs S;
        fill_solve(S, rows, level_blocks(h, w, l), pose_dev, status_dev, stats_dev, nullptr, 0,
                   min_inlier_fraction * (double)A.npix, E_init_host);
        for (int k = 0; k < iterations_host[l]; ++k) {
            S.iter = iter++;
            if (int rc = launch_step(A, S, s)) return rc;
        }
    }
    return 0;
}

OJF_API int ojf_track_associate(const float *depth_dev, const uint8_t *mask_dev, int h, int w, int level,
                                const double *K_host, const float *Kinv_host, const float *model_depth_dev,
                                const float *model_normals_dev, const double *E_ref_host, const double *E_pose_host,
                                double dist_thresh, double angle_thresh_deg, double pyramid_delta,
                                double min_inlier_fraction, void *workspace_dev, size_t workspace_bytes_, double *pose_dev,
                                double *sums_dev, float *jr_dev, uint8_t *reason_dev, int *status_dev, ojf_stream_t stream)
{
    using namespace ojf;
    if (!depth_dev || !K_host || !Kinv_host || !model_depth_dev || !model_normals_dev || !E_ref_host || !E_pose_host ||
        !workspace_dev || !pose_dev || !sums_dev || !status_dev)
        return fail("ojf_track_associate: null pointer argument");
    if (level < 0) return fail("ojf_track_associate: levels must be 1..OJF_TRACK_MAX_LEVELS");
    if (int rc = check_shape("ojf_track_associate", h, w, level + 1)) return rc;
    if (int rc = check_thresholds("ojf_track_associate", dist_thresh, angle_thresh_deg, pyramid_delta, min_inlier_fraction))
        return rc;
    if (workspace_bytes_ < workspace_bytes(h, w, level + 1)) return fail("ojf_track_associate: workspace too small");
    const hipStream_t s = as_stream(stream);
    PyramidArgs P;
    fill_pyramid(P, depth_dev, mask_dev, workspace_dev, h, w, level + 1, pyramid_delta, pose_dev, status_dev, E_pose_host);
    double *rows = (double *)((char *)workspace_dev + pyramid_bytes(h, w, level + 1));
    double *stats = (double *)((char *)workspace_dev + workspace_bytes(h, w, level + 1) - 256);  // the stats row goes to the scratch tail
    AssocArgs A;
    fill_assoc(A, P, level, K_host, Kinv_host, model_depth_dev, model_normals_dev, E_ref_host, dist_thresh,
               angle_thresh_deg, pose_dev, status_dev, rows);
    A.jr = jr_dev;
    A.reason = reason_dev;
    SolveArgs S;
    fill_solve(S, rows, level_blocks(h, w, level), pose_dev, status_dev, stats, sums_dev, 0,
               min_inlier_fraction * (double)A.npix, E_pose_host);
    if (int rc = launch_pyramid(P, s)) return rc;
    return launch_step(A, S, s);
}
