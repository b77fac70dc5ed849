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
// The code of (a) and (b) up to the row (J, r), the host checks and the launch loop are in ojf_track_front.h, which
// ojf_track_rgbd.hip shares; here are the pyramid kernel and the associate kernel that leaves a pixel at its first failed test.
#include "ojf_track_front.h"

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

__global__ __launch_bounds__(kTrackThreads) void track_pyramid_kernel(PyramidArgs A)
{
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g == 0 && A.pose) write_initial_state(A.pose, A.status, A.init);
    if (g >= A.off[A.levels]) return;
    int l = 0;
    while (l + 1 < A.levels && g >= A.off[l + 1]) ++l;
    const int wl = A.w >> l;
    const int pix = g - A.off[l];
    const int r = pix / wl, c = pix % wl;
    const DepthSource S = {A.depth, A.mask, A.w, A.delta};
    float v;
    with_level(l, [&](auto lv) { v = depth_pyramid_value<decltype(lv)::value>(S, r, c); });
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
    LevelCamera cam;
};

// reason code of pixel `pix`, the first test of (b) that fails; for an inlier also J[6] and the residual
__device__ int associate_pixel(const AssocArgs &A, const float R[9], const float t[3], int pix, float J[6], float &res)
{
    const LevelCamera &C = A.cam;
    const int r = pix / C.w, c = pix % C.w;
    const float D = A.D[pix];
    if (D == 0.0f) return 1;
    if (r + 1 >= C.h || c + 1 >= C.w) return 2;
    const float Dd = A.D[pix + C.w], Dr = A.D[pix + 1];
    if (Dd == 0.0f || Dr == 0.0f) return 2;
    float v[3], n[3];
    vertex(C, r, c, D, v);
    if (!live_normal(C, r, c, v, Dd, Dr, n)) return 2;
    float p[3], nw[3], q[3];
    pose_transform(C, R, t, v, n, p, nw, q);
    float ux, uy, fc, fr;
    if (const int stop = project(C, q, ux, uy, fc, fr)) return stop;
    const int mc = (int)fc, mr = (int)fr;
    const int mp = mr * C.w + mc;
    const float dm = A.mdepth[mp];
    if (dm == 0.0f) return 5;
    float g[3];
    if (!model_gap(C, p, mr, mc, dm, g)) return 6;
    const float nm[3] = {A.mnormal[3 * (size_t)mp], A.mnormal[3 * (size_t)mp + 1], A.mnormal[3 * (size_t)mp + 2]};
    if (!normals_agree(C, nw, nm)) return 7;
    plane_row(p, nm, g, J, res);
    return 0;
}

__global__ __launch_bounds__(kTrackThreads) void track_associate_kernel(AssocArgs A)
{
    if (A.status[0] != 0) return;  // a failed step froze the pose: nothing more to do (uniform over the grid)
    float R[9], t[3];
    load_pose_f32(A.pose, R, t);
    double acc[kTrackTerms];
#pragma unroll
    for (int e = 0; e < kTrackTerms; ++e) acc[e] = 0.0;
    // rolled: the measured times (DESIGN.md sections 9 and 25) are this form's; left alone the compiler makes four copies of
    // the body (2.2x the code), which were not measured
#pragma unroll 1
    for (int k = 0; k < kTrackPixPerThread; ++k) {
        const int pix = (int)blockIdx.x * kTrackPixPerBlock + k * kTrackThreads + (int)threadIdx.x;
        if (pix >= A.cam.npix) break;
        float J[6] = {0, 0, 0, 0, 0, 0}, res = 0.0f;
        const int why = associate_pixel(A, R, t, pix, J, res);
        export_row(A.reason, A.jr, pix, why, J, res);
        if (why) continue;
        add_terms(acc, J, res);
    }
    block_terms_to_row(acc, A.rows + (size_t)blockIdx.x * kTrackTerms);
}

// depth pyramid | block rows | 256 bytes (the probe's stats row)
static size_t workspace_bytes(int h, int w, int levels) { return pyramid_bytes(h, w, levels) + rows_bytes(h, w); }

static int check_thresholds(const char *who, double dist, double angle, double delta, double frac)
{
    if (!thresholds_in_range(dist, angle, delta, frac)) return fail(std::string(who) + ": thresholds out of range");
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
    fill_camera(A.cam, P.h, P.w, l, K, Ki, Eref, dist, angle);
}

static int launch_pyramid(const PyramidArgs &P, hipStream_t s)
{
    const int total = P.off[P.levels];
    hipLaunchKernelGGL(track_pyramid_kernel, dim3((total + kTrackThreads - 1) / kTrackThreads), dim3(kTrackThreads), 0, s, P);
    OJF_HIP(hipGetLastError());
    return 0;
}

static int launch_associate(const AssocArgs &A, int blocks, hipStream_t s)
{
    hipLaunchKernelGGL(track_associate_kernel, dim3(blocks), dim3(kTrackThreads), 0, s, A);
    OJF_HIP(hipGetLastError());
    return 0;
}

}  // namespace ojf

OJF_API size_t ojf_track_workspace_bytes(int h, int w, int levels)
{
    using namespace ojf;
    return sizable(h, w, levels) ? workspace_bytes(h, w, levels) : 0;
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
    if (int rc = check_schedule("ojf_track", levels, iterations_host, model_depth_host, model_normals_host)) return rc;
    if (int rc = check_thresholds("ojf_track", dist_thresh, angle_thresh_deg, pyramid_delta, min_inlier_fraction)) return rc;
    if (workspace_bytes_ < workspace_bytes(h, w, levels)) return fail("ojf_track: workspace too small");
    const hipStream_t s = as_stream(stream);
    PyramidArgs P;
    fill_pyramid(P, depth_dev, mask_dev, workspace_dev, h, w, levels, pyramid_delta, pose_dev, status_dev, E_init_host);
    double *rows = (double *)((char *)workspace_dev + pyramid_bytes(h, w, levels));
    AssocArgs A[OJF_TRACK_MAX_LEVELS];
    for (int l = 0; l < levels; ++l)
        fill_assoc(A[l], P, l, K_host, Kinv_host + 9 * l, model_depth_host[l], model_normals_host[l], E_ref_host,
                   dist_thresh, angle_thresh_deg, pose_dev, status_dev, rows);
    if (int rc = launch_pyramid(P, s)) return rc;
    return run_steps(h, w, levels, iterations_host, min_inlier_fraction, rows, pose_dev, status_dev, stats_dev, nullptr,
                     E_init_host, s, [&](int l, int blocks) { return launch_associate(A[l], blocks, s); });
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
    int one_step[OJF_TRACK_MAX_LEVELS] = {};
    one_step[level] = 1;
    if (int rc = launch_pyramid(P, s)) return rc;
    return run_steps(h, w, level + 1, one_step, min_inlier_fraction, rows, pose_dev, status_dev, stats, sums_dev, E_pose_host,
                     s, [&](int, int blocks) { return launch_associate(A, blocks, s); });
}
