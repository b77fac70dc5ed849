/*
 * ojf.h — C ABI of libojf.so, the MI355X (gfx950) implementation of the per-frame hot path of
 * online joint depth fusion + semantics:  extract (ray gather)  ->  fusion net  ->  integrate
 * (scatter).  This is the drop-in boundary: the reference itself has no native layer on this path
 * (SURVEY.md §2.3), so every entry point below names the reference *Python* interface it replaces.
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; ojf_last_error() gives the message of the
 *     calling thread's last failure.  Nothing throws, nothing aborts.
 *   - "dev" pointers are device (HBM) addresses, "host" pointers are ordinary host memory read
 *     before the call returns.  No torch types cross this boundary.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *     is asynchronous; the library never synchronises the device on the hot path.
 *   - volumes are [X,Y,Z] row-major (linear = (ix*Y + iy)*Z + iz, modules/integrator.py:57):
 *     TSDF fp16, weights fp16, semantic ids u8, semantic scores fp16 (modules/database.py:60-76).
 *   - camera: Kinv = inverse(float(K)) row-major f32[9] (modules/extractor.py:39,104),
 *     E = first three rows of the float32 camera-to-world matrix, row-major f32[12]
 *     (modules/extractor.py:40,57,115), origin f64[3] and resolution f64 (modules/database.py:57-58).
 */
#ifndef OJF_H
#define OJF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ojf_stream_t; /* hipStream_t */

/* integrate modes */
#define OJF_MODE_FAST 0   /* order-free fixed-point accumulation; deterministic; TSDF within 1 fp16 ulp */
#define OJF_MODE_PARITY 1 /* per-voxel fp32 sums in the reference's entry order; bit-exact TSDF/weights */

/* activation codes for ojf_conv2d */
#define OJF_ACT_NONE 0
#define OJF_ACT_RELU 1
#define OJF_ACT_LEAKY 2 /* negative slope 0.01 (nn.LeakyReLU default, modules/model.py:12) */
#define OJF_ACT_TANH 3

/* arithmetic of the MFMA kernels of the net (fp32 activations in memory, fp32 accumulation in both) */
#define OJF_ARITH_F32 0   /* v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain */
#define OJF_ARITH_F16X3 1 /* default: operands split into two fp16 halves, three v_mfma_f32_16x16x32_f16 per
                             product block; fp32-class accuracy (drops only lo*lo ~ 2^-22), operands < 65504 */

const char *ojf_version(void);
const char *ojf_last_error(void);
/* number of visible HIP devices, or <0 with ojf_last_error() set (no GPU / no driver) */
int ojf_device_count(void);

/* ---- EXTRACT -------------------------------------------------------------------------------
 * Replaces Extractor.forward (modules/extractor.py:24-79): compute_coordinates (:82-120),
 * extract_values (:309-345), interpolation_weights (:533-593), trilinear_interpolation (:640-681).
 * depth: dev f32[h*w], the UNFILTERED frame (modules/pipeline.py:202).
 * out_values / out_weights: dev f32.  out_layout 0 (rows): element (pixel n, sample k) at
 *   [n*out_stride + k] - the reference's fusion_values / fusion_weights are the out_stride == n_points
 *   case.  out_layout 1 (sample planes): element at [k*out_stride + n], out_stride >= h*w - every store of
 *   a wave is contiguous (the row layout scatters 4-byte stores at a 36-byte pitch: 6x write traffic).
 * pad_value: what out-of-volume corners read for TSDF (-0.1 in the reference, extractor.py:663).
 * Optional debug outputs (NULL to skip) reproduce the other entries of the reference's dict:
 *   dbg_indices i64[h*w,n_points,8,3], dbg_weights f64[h*w,n_points,8], dbg_points f64[h*w,n_points,3],
 *   dbg_pcl f32[h*w,3]. */
int ojf_extract(const float *depth_dev, const float *Kinv_host, const float *E_host,
                const double *origin_host, double resolution, const uint16_t *tsdf_dev,
                const uint16_t *weights_dev, int X, int Y, int Z, int h, int w, int n_points,
                float pad_value, float *out_values_dev, float *out_weights_dev, int out_stride,
                int out_layout, int64_t *dbg_indices_dev, double *dbg_weights_dev, double *dbg_points_dev,
                float *dbg_pcl_dev, ojf_stream_t stream);

/* ---- INTEGRATE -----------------------------------------------------------------------------
 * Replaces Pipeline._prepare_volume_update (modules/pipeline.py:137-171) + Integrator.forward
 * (modules/integrator.py:15-126).  Indices and corner weights are recomputed from depth and pose
 * (bit-identical to ojf_extract) instead of being materialised.
 * depth_filtered: dev f32[h*w] = where(mask, depth, 0) (pipeline.py:196); a pixel integrates iff != 0.
 * est: dev f32, net output for (pixel n, sample k) at [n*est_stride + k]; clamped to +-trunc here.
 * sem_ids u8[h*w] / sem_scores f32[h*w] / id_vol / score_vol: all four non-NULL to run the semantic
 *   update (integrator.py:90-124, "test" mode); all NULL to skip it.
 * workspace: dev memory of ojf_integrate_workspace_bytes(), prepared once by
 *   ojf_integrate_workspace_init(); it is left clean by every call and may be shared by all
 *   scenes of one grid size on one stream.
 * stats_dev (optional, NULL to skip - the counters cost ~14 us per frame of same-line atomics): dev u32[4]
 *   receiving {touched voxels, scatter entries, records (FAST), 0}.
 * Threading / streams: calls that share a workspace must be ordered on one stream (OJF_MODE_FAST alternates two counter
 *   sets per call; which one is next is kept IN the workspace header since round 4, so the call can be captured into a HIP
 *   graph and replayed); distinct workspaces are independent.
 * Range: per frame and voxel the summed corner weight must stay below 2^19 in the 2^-44 fixed point; beyond that the
 *   sums are redone in fp64 and the weight saturates to fp16 infinity like the reference's. */
size_t ojf_integrate_workspace_bytes(int X, int Y, int Z, int h, int w, int n_tail, int mode);
int ojf_integrate_workspace_init(void *workspace_dev, size_t workspace_bytes, int X, int Y, int Z,
                                 int h, int w, int n_tail, int mode, ojf_stream_t stream);
int ojf_integrate(const float *depth_filtered_dev, const float *Kinv_host, const float *E_host,
                  const double *origin_host, double resolution, const float *est_dev,
                  int est_stride, int n_points, int n_tail, float trunc, uint16_t *tsdf_dev,
                  uint16_t *weights_dev, const uint8_t *sem_ids_dev, const float *sem_scores_dev,
                  uint8_t *id_vol_dev, uint16_t *score_vol_dev, int X, int Y, int Z, int h, int w,
                  int mode, void *workspace_dev, size_t workspace_bytes, uint32_t *stats_dev,
                  ojf_stream_t stream);
/* Same, with the validity mask of modules/pipeline.py:196 applied inside the kernels: depth_dev is the RAW frame and
 * mask_dev u8[h*w] (torch bool; NULL = none) marks the valid pixels - torch.where(mask == 0, 0, frame) without its
 * launch.  Bit-identical to ojf_integrate on the filtered frame. */
int ojf_integrate_masked(const float *depth_dev, const uint8_t *mask_dev, const float *Kinv_host, const float *E_host,
                         const double *origin_host, double resolution, const float *est_dev, int est_stride,
                         int n_points, int n_tail, float trunc, uint16_t *tsdf_dev, uint16_t *weights_dev,
                         const uint8_t *sem_ids_dev, const float *sem_scores_dev, uint8_t *id_vol_dev,
                         uint16_t *score_vol_dev, int X, int Y, int Z, int h, int w, int mode, void *workspace_dev,
                         size_t workspace_bytes, uint32_t *stats_dev, ojf_stream_t stream);

/* Entry-list variant with the reference Integrator's own inputs (modules/integrator.py:15-126 fed by
 * Pipeline._prepare_volume_update, modules/pipeline.py:137-171): n_rows = valid pixels x n_tail rows, each
 * with a clamped value f32, 8 corner indices i64[8,3] and 8 corner weights f64[8] (all dev); row_ids u8 /
 * row_scores f32 per row with id_vol / score_vol for the semantic update (all four or none).  FAST
 * accumulation; the workspace is the OJF_MODE_FAST one of a (h*w*n_tail >= n_rows) configuration. */
int ojf_integrate_entries(const float *values_dev, const int64_t *indices_dev, const double *weights_dev,
                          const uint8_t *row_ids_dev, const float *row_scores_dev, int64_t n_rows,
                          uint16_t *tsdf_dev, uint16_t *weights_vol_dev, uint8_t *id_vol_dev,
                          uint16_t *score_vol_dev, int X, int Y, int Z, void *workspace_dev,
                          size_t workspace_bytes, uint32_t *stats_dev, ojf_stream_t stream);

/* ---- FUSION NET ------------------------------------------------------------------------------
 * Replaces FusionNet_v3.forward / FusionNet_v2.forward in eval mode (modules/model.py:164-283)
 * together with Pipeline._prepare_fusion_input / _fusion (modules/pipeline.py:62-102).
 * The host folds every BatchNorm into the preceding convolution and hands the folded layers over
 * in the canonical order documented in DESIGN.md §"net layer order"; the library repacks them for
 * the MFMA kernels and owns that copy plus the activation workspace (sized for h x w). */
typedef struct ojf_net ojf_net;
typedef struct ojf_conv_layer {
    int c_in, c_out, ksize, dilation; /* square kernels, stride 1, padding = dilation*(ksize/2) */
    const float *weight_host;         /* [c_out, c_in, ksize, ksize] fp32, BN folded */
    const float *bias_host;           /* [c_out] fp32, BN folded */
} ojf_conv_layer;

/* version: 2 or 3 (FusionNet_v2 / FusionNet_v3).  n_points = 9, growth = growth_factor - 1 = 5 in
 * every reference config (the YAML files under configs/fusion). */
int ojf_net_create(ojf_net **out, int version, int n_points, int growth, int use_semantics,
                   float output_scale, const ojf_conv_layer *layers_host, int n_layers, int h,
                   int w);
void ojf_net_destroy(ojf_net *net);
/* number of folded conv layers ojf_net_create expects for this topology, <0 if unsupported */
int ojf_net_layer_count(int version, int n_points, int growth, int use_semantics);
/* Packs the net's input from the extractor's row-major outputs (modules/pipeline.py:74-102):
 * channels [0,P) fusion_values, [P,2P) fusion_weights (both f32, laid out as ojf_extract's out_layout
 * `in_layout` with stride `rows_stride`), [2P] the depth
 * frame; with semantics (v3) a second head gets values | weights | (1+sem_id)/n_classes
 * (model.py:274), v2 appends the semantic channel to the single head (model.py:207).  The net's
 * internal activation layout (planes of 4 channels) is private to the library. */
int ojf_net_prepare_input(ojf_net *net, const float *values_dev, const float *weights_dev, int rows_stride,
                          int in_layout, const float *depth_dev, const uint8_t *sem_ids_dev, int n_classes,
                          ojf_stream_t stream);
/* Runs the net; est_dev receives output_scale*tanh(.) for (pixel n, sample k) at [n*est_stride+k]. */
int ojf_net_forward(ojf_net *net, float *est_dev, int est_stride, ojf_stream_t stream);
/* useful multiply-accumulates per pixel of this topology (padding excluded) */
int64_t ojf_net_macs_per_pixel(const ojf_net *net);
/* Kernel launches of the most recent ojf_net_forward on this net (all streams; 0 before the first call). */
int ojf_net_launch_count(const ojf_net *net);
/* The streams the net launches on beside `stream` (the second head of a two-head net, the side streams of the unfused
 * VortexPooling flow), after pairing them with `stream` as the first forward pass would: out[0..2], NULL where there is
 * none; returns how many are non-NULL.  For callers that run other work beside the net (Pipeline's look-ahead pass) and
 * want a stream that shares a hardware queue with none of them (ojf_streams_overlap). */
int ojf_net_side_streams(ojf_net *net, ojf_stream_t stream, ojf_stream_t out[3]);
/* Profiling run of one forward pass (same launches as ojf_net_forward, plus one fence-free HIP event behind every
 * launch): kernel names ('\n'-separated, in launch order) into `names` and each launch's duration in microseconds as
 * its stream saw it (time since the previous launch of that stream completed) into `micros`.  Synchronises the
 * stream.  Returns the number of entries (<= max_entries) or < 0.  For bench.py's per-kernel table; not a hot path. */
int ojf_net_profile(ojf_net *net, float *est_dev, int est_stride, ojf_stream_t stream, char *names, int names_cap,
                    float *micros, int max_entries);
/* The launches a forward pass of a net of this shape consists of, without a device: the kernel names ('\n'-separated, in
 * host enqueue order - the format and order ojf_net_profile reports) into `names`; returns their count or < 0 (bad
 * arguments, a buffer too small for all names).  The pass is planned from the shape alone when a net is created; this
 * entry point runs the same planner with the reference's dilation rates (1, 3, 9, 27).  growth = growth_factor - 1. */
int ojf_net_plan(int version, int n_points, int growth, int use_semantics, int h, int w, int arithmetic, char *names,
                 int names_cap);
/* Arithmetic used by nets created (and ojf_conv2d calls made) AFTER this call: OJF_ARITH_F32 | OJF_ARITH_F16X3.
 * A net keeps the arithmetic it was created with.  Not thread-safe against concurrent ojf_net_create. */
int ojf_net_set_arithmetic(int arithmetic);
/* arithmetic of `net`, or the current default when net == NULL */
int ojf_net_get_arithmetic(const ojf_net *net);
/* Range guard of OJF_ARITH_F16X3.  Every kernel that produces a value a later layer splits into fp16 halves
 * raises a process-wide flag if that value is beyond +-65504 (it cannot be split; a trained, BN-folded FusionNet
 * stays orders of magnitude below).  NaN inputs are not violations: they propagate to NaN outputs as in fp32.
 * ojf_net_forward polls the flag without synchronising and fails once it is set; ojf_net_check synchronises `stream`, returns non-zero (and clears the flag) if it was raised
 * since the last check.  Results produced in between are invalid: switch that network to OJF_ARITH_F32.
 * The volumes are protected: while the flag is set every ojf_integrate / ojf_integrate_masked / ojf_integrate_entries
 * call (both modes) returns 0 without touching a volume - the frame whose net tripped the guard and every frame
 * enqueued after it stay unfused until ojf_net_check has reported (and cleared) the event, so a scene is never
 * corrupted silently; the caller re-fuses those frames after switching the arithmetic (Pipeline does, with
 * FUSION_MODEL.guard_policy = 'f32').  (The reference has no counterpart: its fp32 torch ops have no range limit,
 * modules/pipeline.py:62-72.) */
int ojf_net_check(ojf_stream_t stream);
/* Synchronises `stream`; *flag = 0 none | 1 range violation | 2 internal (dense chain gave up waiting), *skipped = the
 * number of integrate calls skipped since the flag was raised.  Clears nothing (ojf_net_check does).  Either pointer may
 * be NULL. */
int ojf_guard_status(ojf_stream_t stream, int *flag, int *skipped);
/* The flag as the host sees it right now (no synchronisation: what ojf_net_forward tests). */
int ojf_guard_poll(void);
/* 1 when kernels on `a` and `b` run side by side, 0 when the runtime mapped the two streams to one hardware queue (they
 * then take turns: a small round-robin pool of queues backs all streams), < 0 on error.  Synchronises both streams and
 * runs two ~130-us one-wave spin kernels: for set-up code that creates side streams (Pipeline.fuse_many's slot streams,
 * the look-ahead stream of Pipeline.fuse_sequence), not for the frame path.  (No counterpart in the reference, which
 * runs on one stream.) */
int ojf_streams_overlap(ojf_stream_t a, ojf_stream_t b);

/* Stand-alone fused convolution on NHWC fp32 rows (the kernel the net is built from; exported so
 * the parity tests can pin it layer by layer against torch.nn.functional.conv2d).
 * in: [h*w, in_stride], channels [in_off, in_off+c_in); out likewise.  weight [c_out,c_in,k,k]. */
int ojf_conv2d(const float *in_dev, int in_stride, int in_off, float *out_dev, int out_stride,
               int out_off, const ojf_conv_layer *layer_host, int act, int h, int w,
               ojf_stream_t stream);

/* Test entry point: exactly the pool pyramid launch of a VortexPooling in the net's forward pass (same kernel, same grid rule),
 * on caller-supplied device buffers.  Planes: [group][h*w] float4, 16-byte aligned.  z_dev: the entry GEMM's 4*c4 groups, branch
 * b = 1..3 pre-activation = groups [b*c4, (b+1)*c4); q<b>_dev (c4 groups each) = ReLU(pool^b(z) + bias<b>_dev[c4*4]), pool =
 * 3x3 average, zero padding, always / 9.  With z2_dev (two-head nets) z + z2 is pooled and q0_dev = ReLU(z + z2 + bias0_dev) of
 * groups [0, c4).  split_out: the outputs are split planes ({4 fp16 high halves | 4 low halves} per float4).
 * colsums_dev (optional): one block of the launch also folds the global-average branch into the final convolution's bias -
 *   mean[c] = (sum over 16 shards) * 2^-20 / (h*w), NaN where the channel's flag is set, c < cphys
 *   g[t] = bg[t] + sum_c wg_t[c][t] mean[c] (fmaf chain, c ascending; wg_t [cphys][c_out]),
 *   bias_out[t] = bf[t] + sum_j wfg_t[j][t] g[j] (likewise; wfg_t [c_out][c_out]) for t < c_out, 0 for c_out <= t < bias_len
 * - and leaves the sums zeroed.  Both matrices are read as whole float4: 16-byte aligned, allocated up to a multiple of 16 bytes.
 * colsums_dev: int64 fix[16][256] (2^-20 fixed point), then uint32 bad[256].
 * Asynchronous on `stream`. */
int ojf_pool_pyramid(const float *z_dev, const float *z2_dev, float *q1_dev, float *q2_dev, float *q3_dev, float *q0_dev,
                     const float *bias1_dev, const float *bias2_dev, const float *bias3_dev, const float *bias0_dev, int h, int w,
                     int c4, int split_out, void *colsums_dev, const float *wg_t_dev, const float *bg_dev,
                     const float *wfg_t_dev, const float *bf_dev, int cphys, int c_out, float *bias_out_dev, int bias_len,
                     ojf_stream_t stream);

/* Test entry point: the stand-alone branch-entry GEMM of a VortexPooling in the net's forward pass (entry1x1_kernel, the 8-input-tile
 * form in split-fp16 arithmetic), on caller-supplied device buffers.  weight_host [4*cs][c_in_phys] and bias_host [4*cs] are the raw fp32
 * layer (c_in_phys <= 128, cs <= 20, multiples of 4); the call packs them as the net does, runs one launch and synchronises `stream`.
 * Planes: [group][npix] float4, 16-byte aligned; the float4 in front of in_dev must be readable and zero (what lanes outside the frame
 * read).  in_dev: c4_in groups (in_split: split planes, {4 fp16 high halves | 4 low halves} per float4).  out_dev: 5 * 4 groups are
 * computed, groups < og_store (<= cs) are written; ReLU on channels < act_n; groups < split_groups are written as split planes.
 * colsums_dev: int64 fix[16][256] (2^-20 fixed point), then uint32 bad[256] - the launch ADDS the channel sums of its input (which
 * shard a strip adds into is unspecified; the shards' integer sum is not) and sets bad[c] where a 64-pixel strip's sum is not finite.
 * form: 0 = one 64-pixel strip per block, 1 = the persistent form the net launches (a block walks several strips, the next strip's
 * planes in flight while one computes); both give the same bits.  max_blocks: 0 = the net's grid rule, > 0 caps the persistent grid.
 * A stored pre-activation beyond the fp16 range raises the process-wide range guard (ojf_net_check). */
int ojf_entry_gemm(const float *weight_host, const float *bias_host, int c_in_phys, int cs, const float *in_dev, int in_split,
                   int c4_in, int npix, float *out_dev, int og_store, int split_groups, int act_n, void *colsums_dev, int form,
                   int max_blocks, ojf_stream_t stream);

/* Test entry point: one launch of the fused VortexPooling tail in split-fp16 arithmetic (vortex_tail_kernel), on caller-supplied branch
 * planes and raw fp32 layers, which the call packs as the net does; it runs the launch and synchronises `stream`.
 *   t_b = ReLU(w1[b] v_b + b1[b]), y = bf + sum_b wf[:, b*c_out .. (b+1)*c_out) t_b     (b < 4)
 * w1_host [4][c_out][c], b1_host [4][c_out], wf_host [c_out][4*c_out], bf_host [c_out]; c <= 32 branch channels, 113 <= c_out <= 128.
 * v_dev: planes [4 branches][c4 groups][npix] float4 (4*c4 >= c, c4 <= 8), 16-byte aligned; the float4 in front of v_dev must be readable
 * and zero (what lanes outside the frame read).  y is never written; what rides along is:
 * kind 1, the next VortexPooling's entry GEMM: next_w_host [4*cs][c_out], next_b_host [4*cs], next_dims_host = {cs}; out_dev: planes, groups
 *   < og_store (<= cs) of the 5 * 4 computed are written, ReLU on channels < act_n, groups < split_groups as split planes; colsums_dev
 *   (int64 fix[16][256], then uint32 bad[256], see ojf_entry_gemm) gets the channel sums of y added.  rows_stride, rows_n, scale: unused.
 * kind 19, the prediction head: next_dims_host = the 12 channel counts of its 11 pointwise layers (next_dims_host[0] = c_out; in tiles of
 *   16 after rounding up to 4: 8-6-6-5-5-4-4-3-3-2-2-1), next_w_host the layers [c_l+1][c_l] back to back, next_b_host their biases back to
 *   back; LeakyReLU(0.01) between them, out_dev[p * rows_stride + o] = tanh(last layer) * scale for o < rows_n.  og_store, split_groups,
 *   act_n, colsums_dev: unused.
 * form: 1 = the kernel the net launches (branch b + 1's planes requested during branch b, DPP channel sums), 0 = planes requested at
 * each branch's head and __shfl_xor channel sums; both give the same bits.
 * A pre-activation beyond the fp16 range raises the process-wide range guard (ojf_net_check). */
int ojf_vortex_tail(int kind, const float *w1_host, const float *b1_host, const float *wf_host, const float *bf_host, int c, int c_out,
                    const float *next_w_host, const float *next_b_host, const int *next_dims_host, const float *v_dev, int c4, int npix,
                    float *out_dev, int og_store, int split_groups, int act_n, void *colsums_dev, int rows_stride, int rows_n,
                    float scale, int form, ojf_stream_t stream);

/* ---- SEGCONV: convolutions of the 2-D semantic front-end (AdapNet++) ---------------------------
 * One prepacked layer = nn.Conv2d (groups 1, square kernel <= 7, any stride / dilation / zero padding) with what
 * follows it in modules/adapnet.py folded in: eval-mode BatchNorm as scale_host[c_out] (multiplied into the weights)
 * and bias_host[c_out] (either may be NULL), then per call an optional residual add (Bottleneck :33-38 /
 * BottleneckSSMA :60-84), activation act = 0 none | 1 ReLU | 2 sigmoid (SSMA gate :331-337) and an optional
 * elementwise product with mul_dev after the activation (x * link(x), :353).
 * Tensors are NHWC fp32, batch 1 (torch channels_last): pointer to the first channel of pixel 0 + floats per pixel
 * row, so channel slices of a concatenation buffer are addressed in place.  The input rows must hold
 * round_up(c_in, 8) readable, finite channels (the extra ones meet zero weights) and be 16-byte aligned.
 * Output size: floor((h + 2*padding - dilation*(ksize-1) - 1) / stride) + 1 per axis, like torch.
 * Arithmetic: split-fp16 MFMA with fp32 accumulation (see ojf_net_set_arithmetic); the range guard of
 * ojf_net_check covers these launches too.  weight_host is [c_out][c_in][ksize][ksize] (torch layout).
 * act may carry OJF_SEG_ACT_ZERO_PAD: the launch also writes zeros into channels c_out .. round_up(c_out, 8) - 1 of every
 * output row (rows the caller owns with that many floats), which the next layer reads as part of its last group of 8 -
 * instead of a fill launch in front of every such layer. */
#define OJF_SEG_ACT_ZERO_PAD 0x100
typedef struct ojf_segconv ojf_segconv;
int ojf_segconv_create(ojf_segconv **out, const float *weight_host, const float *scale_host, const float *bias_host,
                       int c_in, int c_out, int ksize, int stride, int dilation, int padding);
/* nn.ConvTranspose2d(c_in, c_out, kernel 2*stride, stride, padding stride/2) - the three upsampling layers of the
 * decoder (adapnet.py:226,236,247) - as a 3x3 convolution to stride^2 phase copies of the channels whose store does
 * the pixel shuffle.  weight_host is [c_in][c_out][2*stride][2*stride] (torch layout); scale / bias as above.  Run it
 * with ojf_segconv_forward: h, w are the INPUT size, out_dev is the [h*stride, w*stride] NHWC tensor; no residual /
 * gate.  Deterministic (MIOpen's transposed convolution sums with atomics). */
int ojf_segdeconv_create(ojf_segconv **out, const float *weight_host, const float *scale_host, const float *bias_host,
                         int c_in, int c_out, int stride);
void ojf_segconv_destroy(ojf_segconv *conv);
/* The reference's multi-scale units end in `nn.Dropout(p=0.5)(out)` on a module constructed inside forward(), i.e.
 * ALWAYS in training mode (modules/adapnet.py:80-82): activations are dropped at inference too.  With a state set, the
 * launches of this layer apply that dropout in their epilogue, last (after residual, activation and gate), with
 * rng_state_dev = {seed, frame} (two u64 in device memory, owned by the caller, read at launch time).  Output element
 * (p, c) - pixel p = (b * Ho + y) * Wo + x (batch-major, row-major), channel c < c_out - is kept iff bit 0 of word c % 4
 * of Philox-4x32-10(counter = {p * ceil(c_out / 4) + c / 4, stream_id, frame & 0xffffffff, frame >> 32},
 * key = {seed & 0xffffffff, seed >> 32}) is set (the first word of the counter modulo 2^32).  A kept value v becomes
 * v + v, a dropped one +0.0; pad channels stay 0.  The masks are a pure function of (seed, frame, stream_id, p, c):
 * deterministic, graph-replayable, a fresh draw per frame.  Members of a grouped launch draw with their own stream ids;
 * either every member drops or none does.  advance != 0 instead marks the layer whose launch adds 1 to `frame` (the LAST
 * convolution of a forward pass; no dropout there; member 0 only in a grouped launch).  rng_state_dev == NULL switches
 * both off.  Not for transposed convolutions.  (torch's own generator is not consumed: seed it from torch.initial_seed().) */
int ojf_segconv_set_dropout(ojf_segconv *conv, const unsigned long long *rng_state_dev, unsigned stream_id, int advance);
int ojf_segconv_forward(const ojf_segconv *conv, const float *in_dev, int in_stride, float *out_dev, int out_stride,
                        const float *res_dev, int res_stride, const float *mul_dev, int mul_stride, int act, int h,
                        int w, ojf_stream_t stream);
/* n (1..8) convolutions of one shape - channels, kernel size, stride, frame; dilation / padding may differ as long as the
 * output size agrees - as ONE launch: the two modality encoders of modules/adapnet.py:364-380 in lock-step, the two
 * dilations of a multi-scale unit (:56-73), the three cascades of an eASPP (:175-202).  Arrays of n device pointers
 * (ress / muls: NULL, or per-member pointers); the row strides are common to the members.  Same arithmetic and the same
 * bits per member as n ojf_segconv_forward calls. */
int ojf_segconv_forward_group(int n, const ojf_segconv *const *convs, const float *const *ins_dev, int in_stride,
                              float *const *outs_dev, int out_stride, const float *const *ress_dev, int res_stride,
                              const float *const *muls_dev, int mul_stride, int act, int h, int w, ojf_stream_t stream);
/* The same on `batch` (1..64) images per tensor: every tensor is [batch, h, w, C] NHWC (batch-major, same row stride), the
 * frames of several scenes through the 2-D network at once (Pipeline.fuse_many).  A pixel's result does not depend on
 * the batch it travels in as long as the launch takes the same kernel form (the form is chosen by the number of pixel
 * tiles, and the forms differ in the order they add the K blocks): equal to the single-image call up to that rounding
 * (a few 1e-7 relative).  The weights of a layer are fetched once per launch whatever the batch: on the 15x20 / 30x40
 * maps, where a single frame leaves the matrix pipe idle behind the weight stream, this is what batching buys. */
/* n (1..8) convolutions of DIFFERENT shapes that do not depend on each other, as one launch where their kernel forms allow it
 * (separate launches otherwise; same results either way up to the K-block order of the form): a residual unit's shortcut
 * convolution next to its first 1x1 (modules/adapnet.py:33-38,75-76 run them one after the other), an encoder's skip projection
 * (:142-147) next to the next stage's first layers, the three SSMA blocks of the decoder (:367-369,404-408).  Everything is per
 * member: row strides, residual / gate (NULL entries allowed), act (with OJF_SEG_ACT_ZERO_PAD), input size. */
int ojf_segconv_forward_multi(int n, int batch, const ojf_segconv *const *convs, const float *const *ins_dev, const int *in_strides,
                              float *const *outs_dev, const int *out_strides, const float *const *ress_dev, const int *res_strides,
                              const float *const *muls_dev, const int *mul_strides, const int *acts, const int *hs, const int *ws,
                              ojf_stream_t stream);
int ojf_segconv_forward_batch(const ojf_segconv *conv, int batch, const float *in_dev, int in_stride, float *out_dev, int out_stride,
                              const float *res_dev, int res_stride, const float *mul_dev, int mul_stride, int act, int h,
                              int w, ojf_stream_t stream);
int ojf_segconv_forward_group_batch(int n, int batch, const ojf_segconv *const *convs, const float *const *ins_dev, int in_stride,
                                    float *const *outs_dev, int out_stride, const float *const *ress_dev, int res_stride,
                                    const float *const *muls_dev, int mul_stride, int act, int h, int w, ojf_stream_t stream);

/* ---- FUSION NET, TRAINING (modules/pipeline.py:301-363 with the net in train() mode; csrc/ojf_train.hip) ---------
 * One layer unit of the reference's Sequentials (modules/model.py:4-52,115-141) - conv -> BatchNorm2d (batch
 * statistics) -> activation -> Dropout2d - as device operations on "C4 planes": a tensor with C channels padded to
 * c_phys (multiple of 4) is c_phys/4 planes of float4, element (group cg, pixel p) at [(g0 + cg) * h*w + p]; g0 selects
 * a channel window inside a wider buffer.  The Python wrapper (train.py) turns a unit into one autograd node.
 * Concatenated inputs keep `group`-wide tensors in `slot`-wide slots (19 in 20, 114 in 116): logical input channel j
 * sits at physical channel (j / group) * slot + j % group.
 * ojf_train_packed_floats: floats of a packed weight buffer (0 = unsupported shape).
 * ojf_train_pack: torch weights [OC][IC][k][k] (+ bias [OC]) -> fragment layout of the fp32-MFMA conv kernel, on the
 *   device; transposed != 0 packs the transposed, tap-flipped form whose convolution is the backward-data pass.
 * ojf_train_conv: y = conv(x) + bias on planes (c_out_phys of any size; dilation for 3x3).
 * ojf_train_bn_act: out = drop[c] * scale * act(gamma[c] * (y - mean[c]) * invstd[c] + beta[c]) (has_bn == 0: act(y)).
 *   With has_bn: mean and 1/sqrt(var + eps) per channel are computed here - training != 0: batch statistics (biased
 *   variance, fp64 sums over pixel slabs added in a fixed order) plus the running-statistics update of nn.BatchNorm2d
 *   (momentum, unbiased variance); training == 0: from the running statistics - and returned in mean / invstd for the
 *   backward pass.  partial: ojf_train_partial_doubles(c_phys) doubles of scratch.
 * ojf_train_bn_act_bwd: gradient of that w.r.t. y (batch-statistics form when training != 0), gamma, beta and the
 *   convolution's bias.  accumulate != 0 (here and in ojf_train_wgrad): the parameter gradients are ADDED to the buffers
 *   (gradient accumulation over frames, train_fusion.py:174-189, without a torch add per parameter).
 * ojf_train_wgrad: dW[oc][ic][tap] = sum_p dy[oc][p] * x[ic][p + tap] into torch's layout; partial:
 *   ojf_train_wgrad_partial_floats(...) floats of scratch (pixel slabs, added in slab order: deterministic). */
size_t ojf_train_packed_floats(int c_out_phys, int c_in_phys, int ksize);
int ojf_train_pack(const float *w_dev, const float *bias_dev, int oc, int ic, int ksize, int group, int slot, int c_in_phys,
                   int c_out_phys, int transposed, float *packed_dev, float *bias_packed_dev, ojf_stream_t stream);
int ojf_train_conv(const float *in_dev, int in_g0, int c_in_phys, float *out_dev, int out_g0, int c_out_phys,
                   const float *packed_dev, const float *bias_packed_dev, int ksize, int dilation, int h, int w, ojf_stream_t stream);
/* nn.AvgPool2d(3, 1, 1) on planes (count_include_pad); symmetric: the same call is its backward pass. */
int ojf_train_avgpool3(const float *in_dev, float *out_dev, int c_phys, int h, int w, ojf_stream_t stream);
size_t ojf_train_partial_doubles(int c_phys);
/* per-channel sums of a plane tensor as 64 partial rows [slab][c_phys / 4][8] (sums, then sums of squares), fixed order */
int ojf_train_channel_sums(const float *y_dev, int y_g0, int c_phys, int h, int w, double *partial_dev, ojf_stream_t stream);
int ojf_train_bn_act(const float *y_dev, int y_g0, float *out_dev, int out_g0, int c_phys, int c, int h, int w, const float *gamma_dev,
                     const float *beta_dev, const float *drop_dev, int act, float scale, int has_bn, int training, float momentum,
                     float eps, float *running_mean_dev, float *running_var_dev, double *partial_dev, float *mean_dev,
                     float *invstd_dev, ojf_stream_t stream);
int ojf_train_bn_act_bwd(const float *y_dev, int y_g0, const float *dout_dev, int dout_g0, float *dy_dev, int dy_g0, int c_phys, int c,
                         int h, int w, const float *mean_dev, const float *invstd_dev, const float *gamma_dev, const float *beta_dev,
                         const float *drop_dev, int act, float scale, int has_bn, int training, double *partial_dev,
                         float *dgamma_dev, float *dbeta_dev, float *dbias_dev, int accumulate, ojf_stream_t stream);
size_t ojf_train_wgrad_partial_floats(int c_out_phys, int c_in_phys, int ksize, int h, int w);
int ojf_train_wgrad(const float *x_dev, int x_g0, int c_in_phys, const float *dy_dev, int dy_g0, int c_out_phys, int oc, int ic,
                    int ksize, int dilation, int group, int slot, int h, int w, float *partial_dev, float *dw_dev, int accumulate,
                    ojf_stream_t stream);

/* ---- whole-net TRAINING executor (csrc/ojf_train.hip) -----------------------------------------------------------
 * The net of modules/pipeline.py:322 inside fuse_training and the loss.backward() of train_fusion.py:171 as two calls:
 * forward and backward pass of FusionNet_v3 / _v2 (modules/model.py:164-283) in train() or eval() mode on the layer-unit
 * kernels above, with every activation / gradient buffer owned by the trainer and the four branches of a VortexPooling
 * run as grouped launches.  Parameters, BatchNorm running statistics and gradient tensors stay the caller's: every call
 * receives a table of n_layers = ojf_trainer_layer_count() entries in the layer order of ojf_net_create
 * (v3: block0 (2 per Block) | vortex0 = {global-average conv, 4 x {1x1, 3x3, 3x3, 1x1}, final} | [block2 | vortex2] |
 * vortex3 | pred; v2: block | vortex | vortex_final | pred).
 *   weight [oc][ic][k][k], bias [oc] (or NULL); gamma / beta NULL = no BatchNorm after this convolution;
 *   bn_training: batch statistics + running-statistics update (nn.BatchNorm2d.training of THAT module);
 *   drop_scale: [oc] per-channel Dropout2d factors (0 or 1 / (1 - p)) of this pass, NULL = no dropout;
 *   grad_*: where ojf_trainer_backward writes (accumulate == 0) or adds (accumulate != 0) the parameter gradients.
 * ojf_trainer_forward: values / weights [n_points][h][w], frame [h][w] (+ semantic_frame [h][w] when the net has a
 *   semantic channel) -> est [n_points][h][w] = net(x) * output_scale, all device fp32 NCHW.  weights_epoch: any number
 *   that changes whenever a weight or bias changed (the packed copies are refreshed then).
 * ojf_trainer_backward: d_est [n_points][h][w] -> parameter gradients; exactly one backward per forward (the forward's
 *   activations live in the trainer).  No gradient w.r.t. the inputs is produced (fuse_training's come from the volumes).
 * A trainer serves one stream at a time (its buffers, its side stream and its dy factors are per-trainer state); create one
 * per concurrent training stream.  Frame sizes are arbitrary (no multiple-of-16 requirement). */
typedef struct ojf_trainer ojf_trainer;
typedef struct ojf_train_layer {
    const float *weight, *bias, *gamma, *beta;
    float *running_mean, *running_var;
    float *grad_weight, *grad_bias, *grad_gamma, *grad_beta;
    const float *drop_scale;
    int out_channels, in_channels, ksize, dilation;
    int bn_training, accumulate;
    float momentum, eps;
} ojf_train_layer;
int ojf_trainer_create(ojf_trainer **out, int version, int n_points, int growth, int use_semantics, float output_scale, int h, int w);
void ojf_trainer_destroy(ojf_trainer *t);
/* arithmetic of the convolutions: OJF_ARITH_F16X3 (default; activations must stay inside the fp16 range like in
 * ojf_net_forward - a violation makes the next ojf_trainer_forward fail; the flag STAYS set (it is shared with the inference
 * executors and the integrate calls, which skip while it is set): the caller reports and clears it with ojf_net_check
 * before it continues - a loop that catches the error and carries on without that call has every later ojf_integrate* skip.
 * Pipeline.fuse_training does this before it re-raises) or OJF_ARITH_F32.
 * Under OJF_ARITH_F16X3 backward-data AND the weight gradients run in split-fp16 as well: every dy tensor is stored under a
 * per-unit power-of-two factor that the SAME pass derives from a guaranteed bound on |dy| (max|dz| and max|xhat| collected by
 * the BatchNorm-backward reduction), so gradients of any magnitude stay inside the fp16 range; the factor is divided out
 * exactly by the consumers. */
int ojf_trainer_set_arithmetic(ojf_trainer *t, int arithmetic);
/* arithmetic of the BACKWARD convolutions (backward-data and weight gradients) under a split-fp16 forward:
 * OJF_ARITH_F16X3 (default: as described above) or OJF_ARITH_F32 (every backward pass on the fp32-input MFMA path).
 * Replaces nothing in the reference (loss.backward() of train_fusion.py:171 is fp32 throughout). */
int ojf_trainer_set_backward_arithmetic(ojf_trainer *t, int arithmetic);
int ojf_trainer_layer_count(const ojf_trainer *t);
int ojf_trainer_launch_count(const ojf_trainer *t);
/* Optional replay of the passes as device graphs (default off; ojf_trainer_set_graph turns it on):
 * the launches of a forward / backward pass between the trainer's own buffers and the layer table's tensors are captured once
 * per (layer table contents, arithmetic) on a stream of the trainer's own and replayed with one hipGraphLaunch on the caller's
 * stream - same kernels, same arguments, same bits; a pass is captured the second time its key misses in a row, so a table
 * that changes every frame stays on plain launches.  The launches that touch the per-frame tensors (net input, est, d_est) and
 * the weight packing (weights_epoch) always run as plain launches around the replay.  ojf_trainer_graph_replays: passes served
 * by a replay since create (a test hook).  Replaces nothing in the reference. */
int ojf_trainer_set_graph(ojf_trainer *t, int enable);
int ojf_trainer_graph_replays(const ojf_trainer *t);
int ojf_trainer_forward(ojf_trainer *t, const ojf_train_layer *layers, int n_layers, unsigned long long weights_epoch,
                        const float *values_dev, const float *weights_dev, const float *frame_dev, const float *semantic_frame_dev,
                        float *est_dev, ojf_stream_t stream);
int ojf_trainer_backward(ojf_trainer *t, const ojf_train_layer *layers, int n_layers, const float *d_est_dev, ojf_stream_t stream);

/* The frame step's glue around the net, one launch each instead of ~70 tensor operations:
 * ojf_train_fuse_output(_bwd): modules/pipeline.py:104-127 - fused = (max(w, 0) v + clamp(est, +-init)) / (max(w, 0) + 1) on
 *   the sample planes [n_points][n] (est: net output, v / w: ojf_extract with out_layout 1), gathered at the n_valid pixel
 *   indices valid[] into rows [n_valid][n_points]; backward: d est planes (zero at masked pixels and outside the clamp).
 * ojf_train_fusion_loss(_bwd): utils/loss.py:65-103 FusionLoss on rows [n_valid][n_points] -> *loss_out (device scalar),
 *   including the reference's reshape quirk of the sign-cosine term; fp64 partial sums in fixed order (partial:
 *   ojf_train_loss_partial_doubles(n_valid) doubles of scratch).  Backward: d est rows = *grad_out * d loss / d est. */
int ojf_train_fuse_output(const float *est_planes_dev, const float *values_planes_dev, const float *weights_planes_dev,
                          const long long *valid_dev, int n, int n_points, long long n_valid, float init_value, float *fused_rows_dev,
                          ojf_stream_t stream);
int ojf_train_fuse_output_bwd(const float *d_fused_rows_dev, const float *est_planes_dev, const float *weights_planes_dev,
                              const long long *valid_dev, int n, int n_points, long long n_valid, float init_value,
                              float *d_est_planes_dev, ojf_stream_t stream);
size_t ojf_train_loss_partial_doubles(long long n_valid);
int ojf_train_fusion_loss(const float *est_rows_dev, const float *target_rows_dev, long long n_valid, int n_points, float w_l1, float w_l2,
                          float w_cos, double *partial_dev, float *loss_out_dev, ojf_stream_t stream);
int ojf_train_fusion_loss_bwd(const float *est_rows_dev, const float *target_rows_dev, long long n_valid, int n_points, float w_l1,
                              float w_l2, const float *grad_out_dev, float *d_est_rows_dev, ojf_stream_t stream);

/* ojf_extract writing straight into the fusion net's input planes (values | weights | depth of
 * modules/pipeline.py:74-102), bit-identical to ojf_extract + ojf_net_prepare_input, for nets without a semantic
 * channel and with one head (others: error - use the two calls): no sample planes, no prepare launch. */
int ojf_extract_to_net(const float *depth_dev, const float *Kinv_host, const float *E_host, const double *origin_host,
                       double resolution, const uint16_t *tsdf_dev, const uint16_t *weights_dev, int X, int Y, int Z, int h,
                       int w, int n_points, float pad_value, ojf_net *net, ojf_stream_t stream);

/* ---- one frame of each of SEVERAL scenes as single launches (round 6; Pipeline.fuse_many) ------------------------------
 * modules/extractor.py:24-79 and modules/integrator.py:15-124 for n <= OJF_MAX_SCENES frames of DISTINCT scenes (one frame
 * size, one sample count, one grid size; every job with its own volumes, camera, outputs and integrate workspace): the
 * kernels of ojf_extract / ojf_extract_to_net and of ojf_integrate_masked with the scene as blockIdx.y, so that the
 * dependent-step chains of S frames share one launch ramp and fill the chip while other blocks wait.  Per scene the same
 * blocks run the same code on the same arguments: every output and every volume comes out bit for bit as from the n
 * separate calls.  The reference has no counterpart (its drivers fuse one frame at a time: test_fusion.py:68-80).
 * ojf_extract_job: `net` set = ojf_extract_to_net into that net's input planes (out_* ignored); else out_values /
 *   out_weights with out_stride / out_layout as in ojf_extract.
 * ojf_integrate_job: the arguments of ojf_integrate_masked (mask / semantic pointers NULL where unused, semantics for all
 *   jobs or none); OJF_MODE_FAST only - the PARITY mode's sort is per scene, call ojf_integrate_masked for it. */
#define OJF_MAX_SCENES 8
typedef struct ojf_extract_job {
    const float *depth_dev;
    const float *Kinv_host, *E_host;
    const double *origin_host;
    double resolution;
    const uint16_t *tsdf_dev, *weights_dev;
    ojf_net *net;
    float *out_values_dev, *out_weights_dev;
    int out_stride, out_layout;
} ojf_extract_job;
typedef struct ojf_integrate_job {
    const float *depth_dev;
    const uint8_t *mask_dev;
    const float *Kinv_host, *E_host;
    const double *origin_host;
    double resolution;
    const float *est_dev;
    int est_stride;
    uint16_t *tsdf_dev, *weights_dev;
    const uint8_t *sem_ids_dev;
    const float *sem_scores_dev;
    uint8_t *id_vol_dev;
    uint16_t *score_vol_dev;
    void *workspace_dev;
    size_t workspace_bytes;
} ojf_integrate_job;
int ojf_extract_many(int n, const ojf_extract_job *jobs, int X, int Y, int Z, int h, int w, int n_points, float pad_value,
                     ojf_stream_t stream);
int ojf_integrate_many(int n, const ojf_integrate_job *jobs, int n_points, int n_tail, float trunc, int X, int Y, int Z, int h,
                       int w, ojf_stream_t stream);

/* ---- AdapNet++ front end: the operators around the convolutions (csrc/ojf_seg_ops.hip) --------------------
 * NHWC fp32 rows of batch 1 like ojf_segconv_forward (pointer to channel 0 of pixel 0 + floats per pixel row).
 * ojf_seg_pack_input: modules/pipeline.py:44,50 - three source planes (src[c * chan_stride + p]; chan_stride 0 =
 *   the depth map replicated to three channels) divided by `divisor` (255 for the colour image, 1 for depth) into the
 *   8-channel rows the stem convolution reads (channels 3..7 zero).
 * ojf_seg_maxpool: nn.MaxPool2d(3, 2, 1) of the ResNet stem (modules/adapnet.py:101, torchvision layout).
 * ojf_seg_mean: mean over the pixels per channel (eASPP branch 5 :204-208, Decoder._skip :292-296) -> out[c].
 * ojf_seg_broadcast: out[p][c] = vec[c] (* mul[p][c]): the bilinear upsampling of a 1x1 map / the gated skip.
 * ojf_seg_softmax_max: pipeline.py:57,183 softmax over the classes then max: scores f32[npix], ids u8[npix]; the id is the
 *   first maximum.  A row that holds a NaN or a +Inf, or only -Inf, is all-NaN after the reference's softmax, whose max is
 *   then its first element: score NaN, id 0 (not the index of the NaN / +Inf).
 * ojf_seg_softmax: the whole distribution of the same softmax, probs_dev f32[npix] rows of out_stride >= n_classes floats
 *   (the floats behind the classes are not written): p_c = exp(l_c - l_max) / sum_j exp(l_j - l_max) with
 *   ojf_seg_softmax_max's l_max, summation order and bad-row rule (such a row is NaN in every class).  The largest value of
 *   a row has the bits of ojf_seg_softmax_max's score, and its first arg max is that call's id.
 * ojf_seg_pool_fc: the squeeze chains of eASPP branch 5 (adapnet.py:204-210) and Decoder._skip (:292-296) as two launches
 *   for n (1..8) members: out_m[p][c] = act(bias[c] + sum_k W[c][k] * mean_p' in_m[p'][k]) (* mul_m[p][c]) for every pixel p
 *   of the OUTPUT map - global average (two fixed-order stages), a 1x1 convolution on the 1x1 map in fp32 (W_dev [c_out][c_in],
 *   bias_dev [c_out] or NULL, per member), ReLU (act 1) or none (0), and the broadcast that bilinear upsampling of a 1x1
 *   map is.  partial_dev: n * 128 * c_in floats of scratch. */
int ojf_seg_pack_input(const float *src_dev, int chan_stride, float divisor, int h, int w, float *out_dev, int out_stride,
                       ojf_stream_t stream);
int ojf_seg_maxpool(const float *in_dev, int in_stride, int c, int h, int w, float *out_dev, int out_stride, ojf_stream_t stream);
int ojf_seg_maxpool_batch(int batch, const float *in_dev, int in_stride, int c, int h, int w, float *out_dev, int out_stride,
                          ojf_stream_t stream);  /* [batch, h, w, C] tensors */
int ojf_seg_mean(const float *in_dev, int in_stride, int c, int npix, float *partial_dev /* 32 * c floats of scratch */,
                 float *out_dev, ojf_stream_t stream);
int ojf_seg_broadcast(const float *vec_dev, const float *mul_dev, int mul_stride, int c, int npix, float *out_dev, int out_stride,
                      ojf_stream_t stream);
int ojf_seg_pool_fc(int n, const float *const *ins_dev, int in_stride, int c_in, int npix_in, const float *const *weights_dev,
                    const float *const *biases_dev, int c_out, int act, const float *const *muls_dev, int mul_stride,
                    float *const *outs_dev, int out_stride, int npix_out, float *partial_dev, ojf_stream_t stream);
int ojf_seg_softmax_max(const float *logits_dev, int stride, int n_classes, int npix, float *scores_dev, uint8_t *ids_dev,
                        ojf_stream_t stream);
int ojf_seg_softmax(const float *logits_dev, int stride, int n_classes, int npix, float *probs_dev, int out_stride,
                    ojf_stream_t stream);

/* ---- VOLUME HELPERS (Database) -------------------------------------------------------------
 * ojf_volume_fill_*: Database.reset (modules/database.py:351-370).
 * ojf_volume_filter: Database.filter (:108-112): where weights < value: tsdf = init_value, weights = 0.  The reference
 *   compares its fp16 weights with a Python float, which numpy and torch do in fp16: the test is weights < float16(value).
 *   The call rounds ``threshold`` to fp16 (nearest even) once on the host, so float16(0.1) = 0.0999755859375 is kept by
 *   threshold 0.1 on the device exactly as on the host.
 * ojf_volume_evaluate: utils/metrics.py:111-127 evaluation() on device: with mask = weights > 0 and
 *   est/gt clipped to +-0.04, sums_dev f64[8] receives {n_mask, sum_sq_err, sum_abs_err,
 *   n_intersection(est<0 & gt<0), n_union(est<0 | gt<0), n_sign_equal, 0, 0}.
 * ojf_volume_confusion: Database.evaluate_semantics (:311-349) -> utils/metrics.py:69-108 semantic_evaluation on
 *   device: with mask = weights > 0 and est' = est * mask, gt' = gt * mask, hist_dev u64[n_classes^2] receives the
 *   confusion counts (row = gt', column = est'; flat index gt' * n_classes + est' as in the reference's bincount) and
 *   present_dev u32[512] the label presence flags of est' ([0, 256)) and gt' ([256, 512)).
 * ojf_volume_median5_u8: Database.filter_semantics (:114-116) = scipy.ndimage.median_filter(ids, size=5):
 *   5x5x5 window, 'reflect' boundary, rank-62 element; out must differ from in. */
int ojf_volume_median5_u8(const uint8_t *in_dev, uint8_t *out_dev, int X, int Y, int Z, ojf_stream_t stream);
int ojf_volume_fill_f16(uint16_t *vol_dev, size_t n, float value, ojf_stream_t stream);
int ojf_volume_fill_u8(uint8_t *vol_dev, size_t n, uint8_t value, ojf_stream_t stream);
int ojf_volume_filter(uint16_t *tsdf_dev, uint16_t *weights_dev, size_t n, float threshold,
                      float init_value, ojf_stream_t stream);
int ojf_volume_evaluate(const uint16_t *est_dev, const uint16_t *gt_dev, const uint16_t *weights_dev,
                        size_t n, double *sums_dev, ojf_stream_t stream);
int ojf_volume_confusion(const uint8_t *ids_est_dev, const uint8_t *ids_gt_dev, const uint16_t *weights_dev, size_t n,
                         int n_classes, unsigned long long *hist_dev, uint32_t *present_dev, ojf_stream_t stream);

/* ---- MESH (Database.get_mesh / save 'ply' and 'test' modes) ------------------------------------
 * ojf_mesh_extract: iso-surface of a fused volume as a triangle list, replacing the host-side
 *   skimage.measure.marching_cubes call in modules/database.py:118-139,203-261 and utils/saving.py:42-47.
 *   Marching tetrahedra on the 6-tetrahedra split of every cell (watertight, no ambiguous cases) - same surface up
 *   to the triangulation, NOT the same triangle list as skimage's Lewiner tables.  Cells with a NaN corner or
 *   (weights_dev != NULL) an unobserved corner are skipped.
 *   workspace_dev: ojf_mesh_workspace_bytes(X,Y,Z) bytes of device memory (per-block counts / offsets).  After the
 *   call it holds, as u32 per block of 64 x 4 cells, the offset of the block's first triangle in the list.
 *   Call once with capacity = 0 (vertices may be NULL) to get *count_dev = number of triangles, then again with
 *   buffers of capacity triangles: vertices_dev f32[capacity][3][3] = origin + voxel_index * resolution (origin 0
 *   gives the reference's mesh frame); labels_dev u8[capacity][3] (or NULL) = ids_dev at the voxel nearest to each
 *   vertex, ties to even as np.round does (database.py:124-127; 0 when ids_dev is NULL); keys_dev u64[capacity][3]
 *   (or NULL) = 8 * linear index of the lower voxel of the grid edge the vertex lies on + direction code (bit i set:
 *   the edge advances on axis i) - equal keys <=> same vertex, bit-identical position, so an indexed watertight
 *   mesh is one integer sort away.  *count_dev always receives the full number of triangles; those beyond capacity
 *   are dropped.  No atomics: the triangle order is a pure function of the volume. */
size_t ojf_mesh_workspace_bytes(int X, int Y, int Z);
int ojf_mesh_extract(const uint16_t *tsdf_dev, const uint16_t *weights_dev, const uint8_t *ids_dev, int X, int Y,
                     int Z, float iso, const double *origin_host, double resolution, void *workspace_dev,
                     size_t workspace_bytes, float *vertices_dev, uint8_t *labels_dev, uint64_t *keys_dev,
                     uint32_t capacity, uint32_t *count_dev, ojf_stream_t stream);

/* ojf_points_within: the inner loop of the reconstruction F-score (the reference quotes F-scores, README.md:6, but
 *   holds no code for them - SURVEY.md 0.10; definition in metrics.py / mesh.py).  hit_dev[i] (or NULL) = 1 when a
 *   point of the set lies within tau of query i, *n_hit_dev = number of such queries.  The set arrives binned:
 *   points_sorted_dev f64[M][3] ordered by cell, cell = floor((p - grid_origin) / cell_size) per axis on a
 *   GX x GY x GZ grid (z fastest), cell_start_dev u32[GX*GY*GZ + 1] the offsets; cell_size >= tau.  Queries outside
 *   the grid are legal.  Points and distances are f64 and the test is sqrt(dx^2+dy^2+dz^2) <= tau, the comparison
 *   scipy's cKDTree-based host metric makes, so the counts agree with it. */
int ojf_points_within(const double *query_dev, size_t n_query, const double *points_sorted_dev,
                      const uint32_t *cell_start_dev, const double *grid_origin_host, double cell_size, int GX, int GY,
                      int GZ, double tau, uint8_t *hit_dev, uint32_t *n_hit_dev, ojf_stream_t stream);

/* ---- RENDER (ray casting of a fused volume; no counterpart in the reference's hot path) ---------------------------
 * ojf_render: depth, normal and label images of n views (1 <= n <= OJF_RENDER_MAX_VIEWS, one h x w for all) of the
 *   volume tsdf_dev fp16[X,Y,Z] (X, Y, Z >= 2), KinectFusion-style: each pixel's ray marches from max(box entry, near)
 *   through the trilinear support box of the voxel centres (origin + (i+0.5)*resolution, the frame of extract /
 *   integrate) with steps of max(0.5*resolution, 0.75*max(F,0)) along the ray, and stops at the first sign change
 *   from F > 0 to F <= 0 between two samples whose 8 corners are observed (weights_dev NULL: all are); the hit is the
 *   linear crossing of those two samples.  Kinv_host f32[n][9], E_host f32[n][12] as for ojf_extract; the ray
 *   parameter is the camera z-depth.  Outputs: depth_dev f32[n,h,w] = z-depth of the hit; normals_dev (or NULL)
 *   f32[n,h,w,3] = normalised central difference (+-1 voxel) of the interpolated TSDF at the hit, world frame, pointing
 *   to free space; labels_dev (or NULL; needs ids_dev) u8[n,h,w] = ids_dev at the voxel that contains the hit.  A miss
 *   writes 0 to all three.  Every output element is written once, no atomics: deterministic, the same bits for any n.
 *   The exact fp32 operation order is in csrc/ojf_render.hip. */
#define OJF_RENDER_MAX_VIEWS 64
int ojf_render(const uint16_t *tsdf_dev, const uint16_t *weights_dev, const uint8_t *ids_dev, int X, int Y, int Z,
               const double *origin_host, double resolution, int n, const float *Kinv_host, const float *E_host, int h,
               int w, float near, float *depth_dev, float *normals_dev, uint8_t *labels_dev, ojf_stream_t stream);

/* ---- TRACK (camera pose of a depth frame against the fused model; no counterpart in the reference) -----------------
 * Frame-to-model projective point-to-plane ICP, KinectFusion-style, against ojf_render images of the model at a reference
 *   pose.  Levels l = 0..levels-1 (1 <= levels <= OJF_TRACK_MAX_LEVELS; level l is (h>>l) x (w>>l), every level at least
 *   8 x 8), coarsest first.  depth_dev f32[h*w] (0, negative or non-finite: no depth), mask_dev u8[h*w] or NULL;
 *   K_host f64[9] the level-0 intrinsics (fx_l = fx/2^l, cx_l = (cx+0.5)/2^l - 0.5, likewise y); Kinv_host f32[levels][9]
 *   the inverses the model images were rendered with (fp32(K_l).inverse()); model_depth_host / model_normals_host: host
 *   arrays of `levels` device pointers to the level's ojf_render depth f32[h_l*w_l] and world normals f32[h_l*w_l*3] at
 *   E_ref_host f64[12] (camera-to-world, 3x4 row-major); E_init_host f64[12] the starting pose; iterations_host
 *   int[levels] per level (>= 0, sum <= OJF_TRACK_MAX_ITERATIONS); dist_thresh (m), angle_thresh_deg, pyramid_delta (m),
 *   min_inlier_fraction of a level's pixels.  workspace_dev: >= ojf_track_workspace_bytes(h, w, levels) bytes of device
 *   memory; its first bytes hold the depth pyramid, level after level, f32 row-major.
 *   Outputs: pose_dev f64[12] the tracked camera-to-world pose; stats_dev f64[sum(iterations)][4] per iteration (inlier
 *   count, mean squared residual, |omega|, |tau|); status_dev int[2] {0 | 1 too few inliers | 2 singular system |
 *   3 non-finite step, iteration of the failure or -1}.  After a failure pose_dev holds E_init.  Enqueues
 *   1 + 2*sum(iterations) kernels on `stream` and never waits.  The exact fp32 / fp64 definition is in csrc/ojf_track.hip.
 * ojf_track_associate: one association + solve step at `level` from the pose E_pose_host (the pyramid up to that level is
 *   built in the workspace, sized ojf_track_workspace_bytes(h, w, level + 1)): pose_dev receives the updated pose,
 *   sums_dev f64[OJF_TRACK_TERMS] the reduced terms (21 upper-triangle J_i*J_j, 6 J_i*r, r*r, count), jr_dev (or NULL)
 *   f32[h_l*w_l][7] = (J_0..J_5, r) of every pixel (0 for outliers), reason_dev (or NULL) u8[h_l*w_l] its reason code
 *   (0 inlier, 1 no depth, 2 no normal, 3 behind the reference camera, 4 outside the model image, 5 no model depth,
 *   6 too far, 7 normals disagree), status_dev int[2] as above.  For tests and diagnostics. */
#define OJF_TRACK_MAX_LEVELS 4
#define OJF_TRACK_MAX_ITERATIONS 128
#define OJF_TRACK_TERMS 29
size_t ojf_track_workspace_bytes(int h, int w, int levels);
int ojf_track(const float *depth_dev, const uint8_t *mask_dev, int h, int w, int levels, const double *K_host,
              const float *Kinv_host, const float *const *model_depth_host, const float *const *model_normals_host,
              const double *E_ref_host, const double *E_init_host, const int *iterations_host, double dist_thresh,
              double angle_thresh_deg, double pyramid_delta, double min_inlier_fraction, void *workspace_dev,
              size_t workspace_bytes, double *pose_dev, double *stats_dev, int *status_dev, ojf_stream_t stream);
int ojf_track_associate(const float *depth_dev, const uint8_t *mask_dev, int h, int w, int level, const double *K_host,
                        const float *Kinv_host, const float *model_depth_dev, const float *model_normals_dev,
                        const double *E_ref_host, const double *E_pose_host, double dist_thresh, double angle_thresh_deg,
                        double pyramid_delta, double min_inlier_fraction, void *workspace_dev, size_t workspace_bytes,
                        double *pose_dev, double *sums_dev, float *jr_dev, uint8_t *reason_dev, int *status_dev,
                        ojf_stream_t stream);

/* ---- TRACK RGBD (ojf_track with a photometric term against the model's colour; no counterpart in the reference) -------
 * ojf_track_rgbd: ojf_track's arguments, meaning and outputs, plus image_dev u8[h*w*4] the live colour image (RGBA bytes
 *   as ojf_fuse_color takes them, the fourth ignored), model_color_host: a host array of `levels` device pointers to the
 *   level's ojf_color_render image u8[h_l*w_l*4] at the level's model depth (alpha 0: no colour there), photo_weight
 *   (lambda, metres per intensity level, finite, >= 0; 0 adds no photometric row: ojf_track's bits), photo_thresh
 *   (intensity levels, >= 0: a photometric residual beyond it is cut) and grad_depth_limit (m, > 0: a model intensity
 *   gradient counts only where the model depth of the four axis neighbours is within it of the centre's).  Intensity is
 *   (77 R + 150 G + 29 B) / 256.  A pixel whose geometric reason is 0, 2 or 7 also gets a photometric row
 *   lambda * (J_I, r_I), r_I = I_model(bilinear at its projection) - I_live; the inlier count counts a pixel with either row
 *   once.  workspace_dev: >= ojf_track_rgbd_workspace_bytes(h, w, levels) bytes; with N = sum of h_l*w_l and
 *   P = N*4 rounded up to 256, it holds the depth pyramid f32[N] at 0, the live intensity pyramid f32[N] at P and the
 *   model maps f32[N][4] = (I_m, gx, gy, valid) at 2P, level after level.  Enqueues 1 + 2*sum(iterations) kernels on
 *   `stream` and never waits.  The exact fp32 / fp64 definition is in csrc/ojf_track_rgbd.hip.
 * ojf_track_rgbd_associate: the counterpart of ojf_track_associate (the workspace sized for level + 1 levels; the model
 *   map is written for `level` only): beside jr_dev / reason_dev it exports photo_jr_dev (or NULL) f32[h_l*w_l][7] =
 *   (J_I, r_I) unscaled (0 unless the photometric reason is 0) and photo_reason_dev (or NULL) u8[h_l*w_l]: 0 row added,
 *   1 / 3 / 4 / 5 / 6 as the geometric codes, 8 a bilinear corner is not valid, 9 residual beyond photo_thresh, 10 the
 *   photometric term is off (photo_weight 0).  For tests and diagnostics. */
size_t ojf_track_rgbd_workspace_bytes(int h, int w, int levels);
int ojf_track_rgbd(const float *depth_dev, const uint8_t *mask_dev, const uint8_t *image_dev, int h, int w, int levels,
                   const double *K_host, const float *Kinv_host, const float *const *model_depth_host,
                   const float *const *model_normals_host, const uint8_t *const *model_color_host,
                   const double *E_ref_host, const double *E_init_host, const int *iterations_host, double dist_thresh,
                   double angle_thresh_deg, double pyramid_delta, double min_inlier_fraction, double photo_weight,
                   double photo_thresh, double grad_depth_limit, void *workspace_dev, size_t workspace_bytes,
                   double *pose_dev, double *stats_dev, int *status_dev, ojf_stream_t stream);
int ojf_track_rgbd_associate(const float *depth_dev, const uint8_t *mask_dev, const uint8_t *image_dev, int h, int w,
                             int level, const double *K_host, const float *Kinv_host, const float *model_depth_dev,
                             const float *model_normals_dev, const uint8_t *model_color_dev, const double *E_ref_host,
                             const double *E_pose_host, double dist_thresh, double angle_thresh_deg, double pyramid_delta,
                             double min_inlier_fraction, double photo_weight, double photo_thresh, double grad_depth_limit,
                             void *workspace_dev, size_t workspace_bytes, double *pose_dev, double *sums_dev,
                             float *jr_dev, uint8_t *reason_dev, float *photo_jr_dev, uint8_t *photo_reason_dev,
                             int *status_dev, ojf_stream_t stream);

/* ---- PROJECTIVE (classical voxel-projective TSDF fusion, no network; no counterpart in the reference) ----------------
 * ojf_fuse_projective: fuses n depth views (1 <= n <= OJF_PROJECTIVE_MAX_VIEWS, one h x w for all) into the fp16 volumes
 *   tsdf_dev / weights_dev [X,Y,Z] in place, Curless-Levoy / KinectFusion style: every voxel centre (origin +
 *   (i+0.5)*resolution, the frame of extract / integrate / render) is projected into each view in turn (pixel =
 *   floor(projection + 0.5)); with d the depth there (finite, > 0, mask_dev NULL or non-zero) and zc > near the voxel's
 *   camera depth, s = d - zc; a voxel with -trunc <= s <= trunc (carve == 1: every s >= -trunc, the free space in front of
 *   the surface is pulled to +trunc) takes T = (W*T + min(s, trunc)) / (W + 1), W = min(W + 1, max_weight), rounded to fp16
 *   after every view.  With ids_dev u8 / scores_dev fp16 [X,Y,Z] and labels_dev u8[n,h,w] (all given or all NULL), a
 *   voxel inside the band takes the pixel's label when its score (label_scores_dev f32[n,h,w], NULL: 1.0; rounded to
 *   fp16) is greater than the stored one.  K_host f64[n][9] pinhole intrinsics (entries other than fx, fy, cx, cy must be
 *   0,0,0,0,1), E_host f64[n][12] camera-to-world (rigid; its transpose serves as the inverse).  trunc > 0,
 *   1 <= max_weight <= 2048, near >= 0, carve 0 | 1.  Bad arguments are refused before any HIP call.  Every voxel is
 *   owned by one lane, which walks the views in order: no atomics, no workspace, the same bits on every run, and n views
 *   in one call give the bits of n calls of one view.  Volume pointers that are not 16-byte (ids: 8-byte) aligned are
 *   served by element-wise accesses.  Enqueues one kernel on `stream` and never waits.  The exact fp32 operation order
 *   is in csrc/ojf_projective.hip. */
#define OJF_PROJECTIVE_MAX_VIEWS 32
int ojf_fuse_projective(uint16_t *tsdf_dev, uint16_t *weights_dev, uint8_t *ids_dev, uint16_t *scores_dev,
                        int X, int Y, int Z, const double *origin_host, double resolution, int n,
                        const double *K_host /* f64[n][9] */, const double *E_host /* f64[n][12] */,
                        const float *depth_dev /* f32[n,h,w] */, const uint8_t *mask_dev /* u8[n,h,w] or NULL */,
                        const uint8_t *labels_dev /* u8[n,h,w] or NULL */, const float *label_scores_dev /* or NULL */,
                        int h, int w, float trunc, float max_weight, float near, int carve, ojf_stream_t stream);

/* ---- COLOR (a colour volume beside the fused geometry; no counterpart in the reference) ------------------------------
 * The colour volume color_dev is fp16 [X,Y,Z,4], voxel-major, 8 B per voxel (c0, c1, c2, W): the running mean of the three
 *   image channels on the image's 0..255 scale, in the image's channel order, and the colour weight W (0: no colour yet);
 *   all zeros at reset.
 * ojf_fuse_color: fuses n colour views (1 <= n <= OJF_COLOR_MAX_VIEWS, one h x w for all) into color_dev in place.  Every
 *   voxel centre is projected into each view in turn exactly as ojf_fuse_projective does (same constants, nearest pixel,
 *   depth_dev / mask_dev tests, near); a voxel with -band <= d - zc <= band takes c_k = (W*c_k + image[pixel][k]) / (W + 1),
 *   W = min(W + 1, max_weight), rounded to fp16 after every view.  image_dev u8[n,h,w,4] (4-byte aligned; the 4th byte is
 *   ignored).  band > 0, 1 <= max_weight <= 2048, near >= 0, pinhole K.  The TSDF / weight volumes are not read.  One
 *   owner lane per voxel: no atomics, no workspace, the same bits on every run, and n views in one call give the bits of
 *   n calls of one view.  A pointer off the 16-byte grid is served by element-wise accesses.  One kernel, never waits.
 * ojf_color_sample: rgba_dev u8[n][4] = the colour at points_dev f32[n][3] given in voxel index coordinates (voxel
 *   (i,j,k) sits at (i,j,k)): the trilinear mean over the corners that lie inside the grid and have W > 0, renormalised
 *   by their weights, rounded to u8, alpha 255; (0,0,0,0) where no corner counts or a coordinate is non-finite, < -1 or
 *   > its axis' size.  1 <= n < 2^31.
 * ojf_color_render: rgba_dev u8[n,h,w,4] = the colour at the point of depth depth_dev f32[n,h,w] on each pixel's ray;
 *   n, Kinv_host, E_host, h, w as for ojf_render, whose depth image then reproduces its hit points.  A depth that is not
 *   finite and > 0 writes 0.  Both read-outs use one lane per output and write every output once.
 * Bad arguments are refused before any HIP call.  The exact fp32 operation order is in csrc/ojf_color.hip. */
#define OJF_COLOR_MAX_VIEWS 32
int ojf_fuse_color(uint16_t *color_dev /* fp16 [X,Y,Z,4] */, int X, int Y, int Z, const double *origin_host,
                   double resolution, int n, const double *K_host /* f64[n][9] */, const double *E_host /* f64[n][12] */,
                   const float *depth_dev /* f32[n,h,w] */, const uint8_t *mask_dev /* u8[n,h,w] or NULL */,
                   const uint8_t *image_dev /* u8[n,h,w,4] */, int h, int w, float band, float max_weight, float near,
                   ojf_stream_t stream);
int ojf_color_sample(const uint16_t *color_dev, int X, int Y, int Z, const float *points_dev /* f32[n][3] */, size_t n,
                     uint8_t *rgba_dev /* u8[n][4] */, ojf_stream_t stream);
int ojf_color_render(const uint16_t *color_dev, int X, int Y, int Z, const double *origin_host, double resolution, int n,
                     const float *Kinv_host, const float *E_host, const float *depth_dev, int h, int w,
                     uint8_t *rgba_dev /* u8[n,h,w,4] */, ojf_stream_t stream);

/* ---- LABELS (a per-voxel class distribution and the labels decided from it; no counterpart in the reference) -----------
 * The label volume probs_vol_dev is fp16 [X,Y,Z,S], voxel-major, 16-byte aligned, S = 8 * ceil((n_classes + 1) / 8) for
 *   2 <= n_classes <= 256 (a record of S/8 16-byte chunks per voxel): channels 0..n_classes-1 hold the running mean P_k of
 *   the class probabilities, channel n_classes the weight W (0: nothing fused); all zeros at reset.  The channels behind W
 *   are padding that no call reads or writes.
 * ojf_fuse_label_probs: fuses n views (1 <= n <= OJF_LABEL_MAX_VIEWS, one h x w for all) into probs_vol_dev in place.
 *   Every voxel centre is projected into each view in turn exactly as ojf_fuse_projective does (same constants, nearest
 *   pixel, depth_dev / mask_dev tests, near); a voxel with -band <= d - zc <= band takes, for every class k,
 *   P_k = (W*P_k + p_k) / (W + 1), then W = min(W + 1, max_weight), all rounded to fp16 after every view.  The observation
 *   p comes in exactly one of two forms (the other pointer NULL): probs_dev f32[n,h,w] rows of prob_stride >= n_classes
 *   floats, p_k = the value if it lies in [0, 1], else 0 (a NaN counts as 0); or labels_dev u8[n,h,w], p_k = 1 for the
 *   pixel's label and 0 for the others - a pixel whose label is >= n_classes leaves the voxel alone.  band > 0,
 *   1 <= max_weight <= 2048, near >= 0, pinhole K.  The TSDF / weight volumes are not read.  One owner lane per voxel:
 *   no atomics, no workspace, the same bits on every run, and n views in one call give the bits of n calls of one view.
 *   One kernel, never waits.
 * ojf_label_decide: for every voxel with W > 0, ids_dev u8[X,Y,Z] = the smallest k whose P_k is the largest of the record
 *   and scores_dev fp16[X,Y,Z] = the bits of that P_k; a voxel whose W is 0, -0, negative or NaN keeps its id and score.
 *   One kernel, never waits.
 * Bad arguments (a volume off the 16-byte grid, n_classes outside 2..256, prob_stride < n_classes, both observation forms
 *   or neither, and what ojf_fuse_projective refuses) are refused before any HIP call.  The exact fp32 operation order is
 *   in csrc/ojf_labels.hip. */
#define OJF_LABEL_MAX_VIEWS 32
int ojf_fuse_label_probs(uint16_t *probs_vol_dev /* fp16 [X,Y,Z,S] */, int n_classes, int X, int Y, int Z,
                         const double *origin_host, double resolution, int n, const double *K_host /* f64[n][9] */,
                         const double *E_host /* f64[n][12] */, const float *depth_dev /* f32[n,h,w] */,
                         const uint8_t *mask_dev /* u8[n,h,w] or NULL */, const float *probs_dev /* f32[n,h,w][prob_stride] or NULL */,
                         int prob_stride, const uint8_t *labels_dev /* u8[n,h,w] or NULL */, int h, int w, float band,
                         float max_weight, float near, ojf_stream_t stream);
int ojf_label_decide(const uint16_t *probs_vol_dev, int n_classes, int X, int Y, int Z, uint8_t *ids_dev /* u8 [X,Y,Z] */,
                     uint16_t *scores_dev /* fp16 [X,Y,Z] */, ojf_stream_t stream);

/* ---- RASTER (depth, face, label and colour images of a triangle mesh; the reference renders with OpenGL) --------------
 * ojf_rasterize: n views (1 <= n <= OJF_RASTER_MAX_VIEWS, one h x w for all) of the mesh vertices_dev f32[nv][3] (world
 *   frame) / faces_dev i32[nf][3].  K_host f64[n][9] pinhole intrinsics, E_host f64[n][12] camera-to-world, as for
 *   ojf_fuse_projective; pixel (r, c) has its centre at integer coordinates.  Homogeneous two-sided rasterisation (no
 *   culling, no near-plane clipping: triangles that cross the camera plane come out right): a pixel's ray (rx, ry, 1) hits
 *   a triangle with camera points a, b, c when the edge values e_i = n_i . ray (n0 = b x c, n1 = c x a, n2 = a x b) are all
 *   >= 0 or all <= 0, S = e0 + e1 + e2 != 0 and z = det / S (det = a . n0) is finite and > near.  The pixel keeps the minimum
 *   of (bits(z) << 32) | face index: the nearest hit, ties to the lower face index.  depth_dev f32[n,h,w]: camera z-depth,
 *   0 where nothing is hit; face_dev i32[n,h,w]: the face, -1 where nothing is hit.  A face with an index outside [0, nv)
 *   or a non-finite vertex is skipped.  Edge values of a shared edge negate bit for bit: no holes along shared edges.
 *   keys_dev: u64[n,h,w] workspace (8-byte aligned; its content on return is unspecified).  near >= 0.  Enqueues a fill,
 *   one kernel over (view, triangle) that resolves visibility with a 64-bit atomic minimum - order-independent, the same
 *   bits on every run, and n views in one call give the bits of n calls of one view -, one that spreads the triangles
 *   with large pixel boxes over many waves (their list is kept in depth_dev / face_dev until these are written) and one
 *   that writes the images.
 * ojf_rasterize_attributes: per pixel of face_dev (as ojf_rasterize wrote it, same mesh and views):  labels_dev u8[n,h,w]
 *   = face_labels_dev u8[nf] of the pixel's face, 0 where nothing is hit (both set or both NULL);  rgba_dev u8[n,h,w,4] =
 *   the barycentric mean (lambda_i = e_i / S) of vertex_rgba_dev u8[nv][4] over the face's vertices, bytes 0..2 rounded to
 *   u8, alpha 255, all four bytes 0 where nothing is hit (both set or both NULL; 4-byte aligned).  At least one of the two
 *   outputs.  A face_dev entry outside [0, nf) counts as "nothing is hit".  One kernel.
 * Bad arguments (sizes, n*h*w or 3*nf >= 2^31, a non-pinhole K, non-finite K / E / near, near < 0, null required pointers)
 *   are refused before any HIP call; neither call ever waits.  The exact fp32 operation order is in csrc/ojf_raster.hip. */
#define OJF_RASTER_MAX_VIEWS 32
int ojf_rasterize(const float *vertices_dev /* f32[nv][3] */, int nv, const int *faces_dev /* i32[nf][3] */, int nf, int n,
                  const double *K_host /* f64[n][9] */, const double *E_host /* f64[n][12] */, int h, int w, float near,
                  uint64_t *keys_dev /* u64[n,h,w] workspace */, float *depth_dev /* f32[n,h,w] */,
                  int *face_dev /* i32[n,h,w] */, ojf_stream_t stream);
int ojf_rasterize_attributes(const float *vertices_dev, int nv, const int *faces_dev, int nf, int n, const double *K_host,
                             const double *E_host, int h, int w, const int *face_dev /* i32[n,h,w] */,
                             const uint8_t *face_labels_dev /* u8[nf] or NULL */,
                             const uint8_t *vertex_rgba_dev /* u8[nv][4] or NULL */, uint8_t *labels_dev /* u8[n,h,w] or NULL */,
                             uint8_t *rgba_dev /* u8[n,h,w,4] or NULL */, ojf_stream_t stream);

/* ---- MESH DISTANCE (exact Euclidean distance from voxel centres to a triangle mesh; the reference runs a distance
 *      transform over a voxelised mesh) ----------------------------------------------------------------------------------
 * ojf_mesh_distance: for every voxel of the box (origin_host f64[3], resolution, X, Y, Z; voxel (i, j, k) has its centre
 *   at the fp32 rounding of origin + (index + 0.5) * resolution, the frame of extract / integrate / render /
 *   ojf_fuse_projective) the distance to the mesh vertices_dev f32[nv][3] / faces_dev i32[nf][3] where it is at most band,
 *   and the nearest face.  The squared distance d2 to a triangle is the fp32 minimum of the three segment candidates
 *   (parameter clamped to [0, 1], 0 for an edge of zero length) and, where the triangle has area and the three edge
 *   functions are >= 0, the plane candidate h*h / n.n: a zero-area face is its edges, nothing divides by zero.  A voxel
 *   keeps the minimum of (bits(d2) << 32) | face over the faces with d2 <= (float)band * (float)band: the nearest face, ties
 *   to the lower index.  distance_dev f32[X,Y,Z] = sqrtf(d2), +inf where no face is that near; face_dev i32[X,Y,Z], -1
 *   there.  A face with an index outside [0, nv) or a non-finite vertex is skipped.  The outputs do not depend on how the
 *   triangles are binned or visited: the same bits on every run and for every order of the faces (up to the face index at
 *   exact ties).
 *   Triangles are binned into bricks of 8 x 8 x 8 voxels (count, scan, fill: integer atomics only) and one workgroup per
 *   brick gathers the minimum over its list.  The number of (triangle, brick) pairs is not known in advance: call once with
 *   capacity = 0 (pairs_dev, distance_dev, face_dev may be NULL) to get *count_dev = that number, then again with pairs_dev
 *   u32[capacity], capacity >= that number.  *count_dev (u64, may be NULL) always receives the full number; with a smaller
 *   capacity the lists are cut short, the outputs are unspecified and nothing is written out of bounds.
 *   workspace_dev: ojf_mesh_distance_workspace_bytes(X, Y, Z) bytes (per-brick counts, offsets, cursors), 8-byte aligned.
 *   phases: OJF_MESH_DISTANCE_ALL, or - for measurement - a subset of the phase bits, run in the order bin, scan, fill,
 *   gather on the workspace and the lists that earlier calls with the same arguments left.  Never waits.
 * ojf_mesh_distance_sign: signed_dev f32[X,Y,Z] = +-distance_dev by the angle-weighted pseudonormal of the closest
 *   feature of the voxel's face_dev (same mesh and box as the call that wrote them): the face itself (the sign of h), an
 *   edge (edge_normals_dev f32[ne][3] at face_edges_dev i32[nf][3], entry k for the edge from vertex k to vertex k + 1) or
 *   a vertex (vertex_normals_dev f32[nv][3]); negative where (voxel - closest point) . N < 0, +inf where face_dev < 0.
 *   Positive outside a closed, consistently outward-wound, non-self-intersecting mesh; meaningless for anything else.
 *   One kernel, never waits.
 * Bad arguments (sizes, X*Y*Z or 3*nf >= 2^31, non-finite origin / resolution / band, band <= 0, null required pointers, a
 *   workspace that is too small) are refused before any HIP call.  The exact fp32 operation order is in
 *   csrc/ojf_mesh_distance.hip. */
#define OJF_MESH_DISTANCE_BIN 1
#define OJF_MESH_DISTANCE_SCAN 2
#define OJF_MESH_DISTANCE_FILL 4
#define OJF_MESH_DISTANCE_GATHER 8
#define OJF_MESH_DISTANCE_ALL 15
size_t ojf_mesh_distance_workspace_bytes(int X, int Y, int Z);
int ojf_mesh_distance(const float *vertices_dev /* f32[nv][3] */, int nv, const int *faces_dev /* i32[nf][3] */, int nf,
                      const double *origin_host, double resolution, int X, int Y, int Z, float band, int phases,
                      void *workspace_dev, size_t workspace_bytes, uint32_t *pairs_dev /* u32[capacity] */, uint32_t capacity,
                      uint64_t *count_dev, float *distance_dev /* f32[X,Y,Z] */, int *face_dev /* i32[X,Y,Z] */,
                      ojf_stream_t stream);
int ojf_mesh_distance_sign(const float *vertices_dev, int nv, const int *faces_dev, int nf, const double *origin_host,
                           double resolution, int X, int Y, int Z, const float *distance_dev, const int *face_dev,
                           const float *vertex_normals_dev /* f32[nv][3] */, const float *edge_normals_dev /* f32[ne][3] */,
                           int ne, const int *face_edges_dev /* i32[nf][3] */, float *signed_dev /* f32[X,Y,Z] */,
                           ojf_stream_t stream);

/* ---- RESAMPLE (re-box, resample and merge fused volumes; no counterpart in the reference) ------------------------------
 * Every voxel (i,j,k) of a destination grid [dX,dY,dZ] reads the source grid [sX,sY,sZ] at the index coordinates
 *   g = M (i,j,k) + c (M_host f64[9] row-major, c_host f64[3]; rounded once to fp32; voxel (i,j,k) of the source sits at
 *   g = (i,j,k)): the trilinear mean over the 8 corners around g that lie inside the source grid, have a trilinear weight
 *   > 0 and are observed (source weight > 0; every in-grid corner when there is no weight volume), renormalised by the sum
 *   ws of their trilinear weights.  A voxel is covered when ws >= 0.5 and its new weight does not round to +0; a g with a
 *   coordinate that is non-finite, < -1 or > its axis' size covers nothing.  For a rigid map x_s = R x_d + t between the
 *   boxes, M = R res_d / res_s and c = (R (origin_d + res_d / 2) + t - origin_s) / res_s - 1/2.
 * ojf_resample_volumes: the fp16 TSDF, fp16 weights (both NULL: the ground-truth form, every voxel observed), u8 ids and
 *   fp16 scores (all four set or all four NULL) of a scene.  T' and W' are the renormalised means of the counting corners;
 *   id' and score' are those of the counting corner with the largest trilinear weight (the first of equals in corner order
 *   000..111, bits x, y, z).
 * ojf_resample_records: a record volume fp16 [X,Y,Z,S] whose channel Cw is the weight - the colour volume (S = 4, Cw = 3;
 *   2-byte aligned) or a label volume (S a multiple of 8 up to 264, Cw = n_classes; 16-byte aligned).  Channels 0..Cw-1
 *   take the renormalised mean, channel Cw the mean weight; channels behind Cw are neither read nor written.
 * mode OJF_RESAMPLE_REPLACE: every destination voxel is written once; an uncovered one takes init_value, weight 0, id 0,
 *   score 0 (record channels 0..Cw: 0).  mode OJF_RESAMPLE_MERGE (needs the weight volumes): an uncovered voxel is left
 *   alone; a covered one takes the running mean T = (W_d T_d + W' T') / (W_d + W') (T' where W_d == 0),
 *   W = min(W_d + W', max_weight), and id' / score' where score' > score_d.  1 <= max_weight <= 65504 in both modes.
 * One lane (a group of lanes for records of 4 chunks and more) per destination voxel: no atomics, no workspace, the same
 *   bits on every run.  One kernel each, never waits.  Bad arguments (null or mismatched pointers, non-positive sizes,
 *   more than 2^31-1 voxels, a source that overlaps a destination in memory, non-finite M / c / init_value, an unknown
 *   mode, max_weight, S, Cw, alignment) are refused before any HIP call.  The exact fp32 operation order is in
 *   csrc/ojf_resample.hip. */
#define OJF_RESAMPLE_REPLACE 0
#define OJF_RESAMPLE_MERGE 1
int ojf_resample_volumes(const uint16_t *src_tsdf_dev, const uint16_t *src_weights_dev /* or NULL */,
                         const uint8_t *src_ids_dev /* or NULL */, const uint16_t *src_scores_dev /* or NULL */, int sX, int sY,
                         int sZ, uint16_t *dst_tsdf_dev, uint16_t *dst_weights_dev, uint8_t *dst_ids_dev, uint16_t *dst_scores_dev,
                         int dX, int dY, int dZ, const double *M_host /* f64[9] */, const double *c_host /* f64[3] */,
                         float init_value, int mode, float max_weight, ojf_stream_t stream);
int ojf_resample_records(const uint16_t *src_dev /* fp16 [sX,sY,sZ,S] */, int sX, int sY, int sZ,
                         uint16_t *dst_dev /* fp16 [dX,dY,dZ,S] */, int dX, int dY, int dZ, int S, int Cw,
                         const double *M_host /* f64[9] */, const double *c_host /* f64[3] */, int mode, float max_weight,
                         ojf_stream_t stream);

/* ---- CONNECTED COMPONENTS (floater removal, 3-D instances; no counterpart in the reference) ----------------------------
 * ojf_volume_components: the connected components of the foreground of an [X,Y,Z] volume (linear index v = (x Y + y) Z + z).
 *   mask_dev u8 (NULL: every voxel) - foreground where the byte is non-zero; keys_dev u8 (NULL: all equal) - neighbouring
 *   foreground voxels are joined only when their key bytes are equal; connectivity 6 (faces) or 26 (the 3x3x3 neighbourhood).
 *   labels_dev i32[X,Y,Z]: -1 on the background, else the smallest linear index of the voxel's component (its root).
 *   The list, in ascending order of root, n entries: roots_dev i32, sizes_dev i32 (voxels), list_keys_dev u8 (the key byte at
 *   the root, 0 without keys), boxes_dev i32[6] = (x0, y0, z0, x1, y1, z1), inclusive.  ids_dev i32[X,Y,Z]: -1 on the
 *   background, else the rank 0..n-1 of the voxel's component in the list.  *count_dev = n.  Everything is a function of the
 *   input alone - integer atomics only, and the root is a minimum: the same bits on every run.
 *   phases: OJF_COMPONENTS_ALL, or a subset run in the order brick (union-find per 4 x 4 x 64 brick in LDS), seam (unions
 *   across brick faces, edges and corners with agent-scope atomics only; no thread waits for another workgroup), flatten
 *   (labels), rank (ids, *count_dev), list (the list arrays) on the outputs and the workspace that earlier calls with the same
 *   arguments left.  n is not known in advance: call with capacity = 0 (the list arrays may be NULL; the list phase does
 *   not run and nothing is written to them) to get labels, ids and n, then with phases = OJF_COMPONENTS_LIST and arrays of
 *   capacity >= n entries; a single call with enough capacity does both.  Entries beyond capacity are dropped.
 *   workspace_dev: ojf_volume_components_workspace_bytes(X, Y, Z) bytes, 8-byte aligned (4 bytes per voxel and a little).
 * ojf_volume_observed_mask: mask_dev[v] = 1 where fp32(weights[v]) > 0 and tsdf[v] is not a NaN (the mesh extractor's
 *   observed voxel: a NaN, negative or -0 weight is unobserved) and, with use_band != 0, |fp32(tsdf[v])| < band; else 0.
 * ojf_volume_components_apply: where ids_dev[v] is in [0, n_components) and keep_dev[ids_dev[v]] == 0: tsdf = init_value,
 *   weights = 0 - what ojf_volume_filter writes.  Every other voxel is not written at all.
 * All launches go on the caller's stream and never wait.  Bad arguments (null required pointers, non-positive sizes,
 *   X*Y*Z >= 2^31, a connectivity other than 6 and 26, unknown phases, a workspace that is too small, alignment, a band that
 *   is not > 0) are refused before any HIP call.  The kernels are described in csrc/ojf_components.hip. */
#define OJF_COMPONENTS_BRICK 1
#define OJF_COMPONENTS_SEAM 2
#define OJF_COMPONENTS_FLATTEN 4
#define OJF_COMPONENTS_RANK 8
#define OJF_COMPONENTS_LIST 16
#define OJF_COMPONENTS_ALL 31
size_t ojf_volume_components_workspace_bytes(int X, int Y, int Z);
int ojf_volume_components(const uint8_t *mask_dev /* or NULL */, const uint8_t *keys_dev /* or NULL */, int X, int Y, int Z,
                          int connectivity, int phases, void *workspace_dev, size_t workspace_bytes, int32_t *labels_dev,
                          int32_t *ids_dev, int32_t *roots_dev, int32_t *sizes_dev, uint8_t *list_keys_dev,
                          int32_t *boxes_dev /* i32[capacity][6] */, uint32_t capacity, uint32_t *count_dev, ojf_stream_t stream);
int ojf_volume_observed_mask(const uint16_t *tsdf_dev, const uint16_t *weights_dev, size_t n, int use_band, float band,
                             uint8_t *mask_dev, ojf_stream_t stream);
int ojf_volume_components_apply(const int32_t *ids_dev, const uint8_t *keep_dev, uint32_t n_components, uint16_t *tsdf_dev,
                                uint16_t *weights_dev, size_t n, float init_value, ojf_stream_t stream);

/* ---- DISTANCE TRANSFORM (exact Euclidean distance and nearest seed of every voxel; surface voxels and ESDF of a fused TSDF) ----
 * Volumes are [X,Y,Z], linear index v = (x Y + y) Z + z, 1 <= X, Y, Z <= 2048 and X*Y*Z < 2^31.
 * ojf_volume_edt: seeds_dev u8 - a voxel is a seed where the byte is non-zero.  dist2_dev i32[X,Y,Z]: the minimum over the
 *   seeds q of |p - q|^2 in voxel units; nearest_dev i32[X,Y,Z]: the smallest linear index among the seeds that attain it -
 *   the pair is the minimum of the 64-bit key (d^2 << 32) | index(q), a function of the input alone.  With no seed in reach
 *   dist2 = OJF_EDT_NONE and nearest = -1.  max_dist2 (negative: unlimited): a voxel with d^2 > max_dist2 gets NONE / -1, every
 *   other voxel is unchanged from the unlimited result; no pass then looks further than sqrt(max_dist2) along its axis.
 *   phases: OJF_EDT_ALL, or a subset run in the order z, y, x on the outputs and the workspace that earlier calls with the
 *   same arguments left (each is a 1-D pass along its axis; ties go to the smaller coordinate).
 *   workspace_dev: ojf_volume_edt_workspace_bytes(X, Y, Z) bytes, 8-byte aligned (4 bytes per voxel).
 * ojf_volume_surface_mask: mask_dev[v] = 1 where v is observed as ojf_volume_observed_mask defines it without a band and has
 *   an observed face neighbour on the other side of the surface (inside: fp32(tsdf) < 0; -0.0 and +0.0 are outside); else 0.
 * ojf_volume_esdf: esdf_dev[v] = s (fp32(resolution) sqrtf((float)dist2[v])), each operation correctly rounded, s = -1 where
 *   v is observed and inside, else +1; where dist2[v] is OJF_EDT_NONE, s far (far >= 0, +inf allowed).
 * All launches go on the caller's stream and never wait.  Bad arguments (null pointers, a dimension out of range, unknown
 *   phases, a workspace that is too small, alignment, a resolution that is not > 0 and finite, a far that is not >= 0) are
 *   refused before any kernel is launched and leave every output untouched.  The kernels are described in
 *   csrc/ojf_distance.hip. */
#define OJF_EDT_Z 1
#define OJF_EDT_Y 2
#define OJF_EDT_X 4
#define OJF_EDT_ALL 7
#define OJF_EDT_NONE 0x7fffffff
size_t ojf_volume_edt_workspace_bytes(int X, int Y, int Z);
int ojf_volume_edt(const uint8_t *seeds_dev, int X, int Y, int Z, int max_dist2, int phases, void *workspace_dev,
                   size_t workspace_bytes, int32_t *dist2_dev, int32_t *nearest_dev, ojf_stream_t stream);
int ojf_volume_surface_mask(const uint16_t *tsdf_dev, const uint16_t *weights_dev, int X, int Y, int Z, uint8_t *mask_dev,
                            ojf_stream_t stream);
int ojf_volume_esdf(const int32_t *dist2_dev, const uint16_t *tsdf_dev, const uint16_t *weights_dev, size_t n, float resolution,
                    float far, float *esdf_dev, ojf_stream_t stream);

/* ---- MESH SIMPLIFICATION (vertex clustering with quadric error metrics; definition: DESIGN.md §19, tests/simplify_ref.py) ----
 * vertices_dev f32[nv][3], faces_dev i32[nf][3]; 1 <= nv < 2^31, 0 <= nf <= 2^24 (the exact integer sums are proved for that
 * many faces).  The grid: lo_host f32[3] finite, cell > 0 and finite, GX, GY, GZ >= 1 with GX*GY*GZ < 2^31.  A vertex is valid
 * when t = (v - lo) / cell is finite and 0 <= floorf(t) < G on every axis; all valid vertices of one cell become ONE output
 * vertex (a cluster), the clusters are numbered by ascending cell index (gx GY + gy) GZ + gz.  The output vertex lies where the
 * summed plane quadric of the incident faces, plus a small pull towards the vertex mean, is smallest; source_dev[c] is the input
 * vertex of cluster c nearest to it (the lower index at a tie), to carry labels and colours.  Face f becomes
 * (cluster[v0], cluster[v1], cluster[v2]) and is kept when its indices are in range, its vertices valid, its fp32 area neither
 * 0 nor non-finite and its three clusters differ; kept faces stay in input order, face_source_dev[j] is the input face.
 * The same bits on every run and for every order of the faces (all sums are exact integers).
 * Two calls, like ojf_mesh_extract: phases MARK|SCAN|COUNT write counts_dev[0] = clusters and counts_dev[1] = kept faces and
 *   touch no output; the host reads them, allocates out_vertices_dev f32[vertex_capacity][3], source_dev i32[vertex_capacity],
 *   out_faces_dev i32[face_capacity][3], face_source_dev i32[face_capacity] and clusters_dev of
 *   ojf_mesh_simplify_cluster_bytes(counts[0]) bytes (128 per cluster, 128-byte aligned), and calls again with
 *   ACCUMULATE|SOLVE|NEAREST|FACES and the same other arguments.  Any subset of the phase bits runs, in that order, on what
 *   earlier calls left in workspace_dev, clusters_dev and counts_dev.  Nothing is written past a capacity, and no cluster past
 *   clusters_bytes / 128 is touched.
 * workspace_dev: ojf_mesh_simplify_workspace_bytes(nv, nf, GX, GY, GZ) bytes, 8-byte aligned; 0 for sizes out of range.
 * All launches go on the caller's stream and never wait.  Bad arguments (sizes out of range, nf > 2^24, unknown phases, null
 *   required pointers, a short workspace, alignment, a cell that is not > 0 and finite, a non-finite lo) are refused before any
 *   HIP call and leave every output untouched.  The kernels are described in csrc/ojf_simplify.hip. */
#define OJF_SIMPLIFY_MARK 1
#define OJF_SIMPLIFY_SCAN 2
#define OJF_SIMPLIFY_COUNT 4
#define OJF_SIMPLIFY_ACCUMULATE 8
#define OJF_SIMPLIFY_SOLVE 16
#define OJF_SIMPLIFY_NEAREST 32
#define OJF_SIMPLIFY_FACES 64
#define OJF_SIMPLIFY_ALL 127
size_t ojf_mesh_simplify_workspace_bytes(int nv, int nf, int GX, int GY, int GZ);
size_t ojf_mesh_simplify_cluster_bytes(uint32_t nc);
int ojf_mesh_simplify(const float *vertices_dev, int nv, const int32_t *faces_dev, int nf, const float *lo_host, float cell, int GX,
                      int GY, int GZ, int phases, void *workspace_dev, size_t workspace_bytes, void *clusters_dev,
                      size_t clusters_bytes, float *out_vertices_dev, int32_t *source_dev, uint32_t vertex_capacity,
                      int32_t *out_faces_dev, int32_t *face_source_dev, uint32_t face_capacity, uint32_t *counts_dev,
                      ojf_stream_t stream);

/* ---- REGISTER (the rigid transform between two fused scenes; definition: csrc/ojf_register.hip) ----------
 * Volume-to-volume registration on signed distance fields.  The MOVING scene is an fp16 TSDF [mX,mY,mZ] (metres) with its
 * weights, the FIXED scene either an fp16 TSDF + weights [fX,fY,fZ] (fixed_field_dev NULL) or an f32 field [fX,fY,fZ] in metres
 * (fixed_tsdf_dev and fixed_weights_dev NULL; a non-finite voxel is "no value").  Origins f64[3] and resolutions are those of
 * the volume frame (voxel (i,j,k) has its centre at origin + (i+0.5, j+0.5, k+0.5) resolution) and are rounded to fp32: callers
 * shift both worlds so that the scenes lie about their origins (registration.py does).  The pose P f64[12] (3x4 row-major) maps
 * points of the moving world to the fixed world - the `transform` of ojf_resample_volumes with destination = moving.
 * ojf_register_select: the points of a volume - voxels whose three indices are multiples of `stride` (>= 1), that are observed
 *   (weight > 0, TSDF not NaN) and have |TSDF| < band (> 0) - as u32 linear indices in increasing order.  count_dev[0] receives
 *   their number; list_dev (or NULL: count only) the first `capacity` of them.  workspace_dev:
 *   ojf_register_workspace_bytes(X*Y*Z) bytes, 4-byte aligned.
 * ojf_register_workspace_bytes(n): the workspace of ojf_register / ojf_register_associate for n points (8-byte aligned), which
 *   also serves ojf_register_select on a volume of n voxels; 0 for n = 0 or n >= 2^31.
 * ojf_register: `iterations` Gauss-Newton steps (one associate + one solve launch each) of one stage on the points list_dev
 *   u32[n_points] of the moving volume.  field_band: a point where |field| >= field_band is no inlier (pass +inf for an f32
 *   field); dist: nor is one whose residual exceeds dist.  pose_dev f64[12] in/out: continue_from_pose == 0 starts from
 *   E_init_host (one more launch writes it and status {0, -1}); otherwise the call continues from what pose_dev and status_dev
 *   hold.  stats_dev f64[OJF_REGISTER_MAX_ITERATIONS][4]: rows first_iteration .. first_iteration + iterations - 1 are written
 *   (inlier count, mean squared residual, |omega|, |tau|); status_dev int[2] {0 | 1 fewer inliers than
 *   min_inlier_fraction n_points | 2 singular system | 3 non-finite step, iteration of the failure or -1}.  A failed step always
 *   restores E_init_host and freezes the rest (later stats rows are 0).  Never waits.
 * ojf_register_associate: one step from the host pose E_pose_host: pose_dev the updated pose, sums_dev f64[OJF_TRACK_TERMS],
 *   jr_dev (or NULL) f32[n_points][7] = (J_0..J_5, r) of every point (0 for outliers), reason_dev (or NULL) u8[n_points]
 *   (0 inlier, 1 outside the fixed grid, 2 a corner without a value, 3 field saturated, 4 residual too large, 5 no gradient).
 *   For tests and diagnostics.
 * Bad arguments - a malformed box, a non-finite origin or resolution, stride < 1, a band, field_band or dist that is not > 0,
 *   n_points == 0, misaligned or null pointers, a short workspace - are refused before any HIP call, with a text that names the
 *   argument. */
#define OJF_REGISTER_MAX_ITERATIONS 128
size_t ojf_register_workspace_bytes(size_t n);
int ojf_register_select(const uint16_t *tsdf_dev, const uint16_t *weights_dev, int X, int Y, int Z, float band, int stride,
                        void *workspace_dev, size_t workspace_bytes, uint32_t *list_dev /* or NULL */, uint32_t capacity,
                        uint32_t *count_dev, ojf_stream_t stream);
int ojf_register(const uint16_t *moving_tsdf_dev, int mX, int mY, int mZ, const double *moving_origin_host,
                 double moving_resolution, const uint32_t *list_dev, uint32_t n_points, const uint16_t *fixed_tsdf_dev,
                 const uint16_t *fixed_weights_dev, const float *fixed_field_dev, int fX, int fY, int fZ,
                 const double *fixed_origin_host, double fixed_resolution, double field_band, double dist, int iterations,
                 int first_iteration, double min_inlier_fraction, const double *E_init_host, int continue_from_pose,
                 void *workspace_dev, size_t workspace_bytes, double *pose_dev, double *stats_dev, int *status_dev,
                 ojf_stream_t stream);
int ojf_register_associate(const uint16_t *moving_tsdf_dev, int mX, int mY, int mZ, const double *moving_origin_host,
                           double moving_resolution, const uint32_t *list_dev, uint32_t n_points, const uint16_t *fixed_tsdf_dev,
                           const uint16_t *fixed_weights_dev, const float *fixed_field_dev, int fX, int fY, int fZ,
                           const double *fixed_origin_host, double fixed_resolution, double field_band, double dist,
                           double min_inlier_fraction, const double *E_pose_host, void *workspace_dev, size_t workspace_bytes,
                           double *pose_dev, double *sums_dev, float *jr_dev, uint8_t *reason_dev, int *status_dev,
                           ojf_stream_t stream);

/* ---- TVL1 (robust fusion of depth views: per-voxel histograms and their TV-L1 minimiser; definition: csrc/ojf_tvl1.hip,
 * DESIGN.md §22; the reference's counterpart is deps/mesh-fusion/libfusiongpu/fusion_zach_tvl1.cu) -------------------------
 * The histogram volume hist_dev is fp16 [X,Y,Z,S], voxel-major, 16-byte aligned, S = 8 * ceil((n_bins + 1) / 8) for
 *   2 <= n_bins <= OJF_HIST_MAX_BINS (one or two 16-byte chunks per voxel) - the record layout of the label volume: channels
 *   0..n_bins-1 hold the running means h_b of the votes, channel n_bins the weight W (0: never observed); all zeros at reset;
 *   the channels behind W are padding that no call reads or writes.  Bin b has its centre at the normalised distance
 *   l_b = 2b / (n_bins - 1) - 1 (-1: -trunc, +1: +trunc).
 * ojf_fuse_depth_hist: fuses n views (1 <= n <= OJF_HIST_MAX_VIEWS, one h x w for all) into hist_dev in place.  Every voxel
 *   centre is projected into each view in turn exactly as ojf_fuse_projective does (same constants, nearest pixel, depth_dev /
 *   mask_dev tests, near).  With s = d - zc, a view votes when s >= -trunc (carve == 1: free space in front of a surface votes
 *   the last bin) or when -trunc <= s <= trunc (carve == 0); the vote is split linearly over the two bins that bracket
 *   t = min(s, trunc) / trunc, the nearer bin taking the larger share; h_b = (W*h_b + vote_b) / (W + 1), then
 *   W = min(W + 1, max_weight), rounded to fp16 after every view.  trunc > 0, 1 <= max_weight <= 2048, near >= 0, pinhole K.
 *   One owner lane per voxel: no atomics, no workspace, the same bits on every run, and n views in one call give the bits of
 *   n calls of one view.  One kernel, never waits.
 * ojf_tvl1_workspace_bytes: the workspace of ojf_tvl1_solve for a box (about 33 bytes per voxel); 0 for a box it refuses.
 * ojf_tvl1_solve: `iterations` (>= 0) Chambolle-Pock iterations towards the minimiser of
 *   TV(u) + lambda * sum_voxels sum_b h_b |u - l_b| over the observed voxels (W > 0) of hist_dev.  An edge between two
 *   6-neighbours counts when both are observed and inside the box (a Neumann boundary everywhere else); unobserved voxels are
 *   never written and never influence an observed one.  u_dev f32 [X,Y,Z] (16-byte aligned, normalised distance in [-1, 1])
 *   is the caller's: read and written at the observed voxels only.  lambda > 0; tau, sigma > 0 with tau * sigma <= 1/12.
 *   restart: OJF_TVL1_RESTART runs the set-up pass (the edge bits, the list of the bricks that hold an observed voxel), zeroes
 *   the dual and sets u of every observed voxel to clamp(sum_b h_b l_b / sum_b h_b); OJF_TVL1_CONTINUE goes on from u_dev and
 *   the workspace as the previous call on the same hist_dev and box left them - N iterations in one call give the bits of any
 *   split of N over consecutive calls; OJF_TVL1_REFRESH says that hist_dev has changed since (views were fused): the set-up
 *   pass runs again, a voxel observed for the first time starts at its clamp(...) value with a zero dual, the others go on.
 *   Or-ing OJF_TVL1_ALL_BRICKS into _RESTART / _REFRESH lists every brick of the box (the same bits; for measurements).
 *   workspace_dev: ojf_tvl1_workspace_bytes bytes, 256-byte aligned, owned by the (hist_dev, u_dev) pair between calls.
 *   Two launches for the set-up, one per iteration, all on `stream`; never waits.
 * ojf_tvl1_write: for every observed voxel, tsdf_dev fp16 [X,Y,Z] = trunc * u and weights_dev fp16 [X,Y,Z] = W; every other
 *   voxel keeps what it holds.  One kernel, never waits.
 * Bad arguments (hist_dev off the 16-byte grid, n_bins outside 2..OJF_HIST_MAX_BINS, tau * sigma > 1/12, lambda <= 0,
 *   negative iterations, a misaligned or short workspace, and what ojf_fuse_projective refuses) are refused before any HIP
 *   call.  The exact fp32 operation order is in csrc/ojf_tvl1.hip. */
#define OJF_HIST_MAX_BINS 15
#define OJF_HIST_MAX_VIEWS 32
#define OJF_TVL1_CONTINUE 0
#define OJF_TVL1_RESTART 1
#define OJF_TVL1_REFRESH 2
#define OJF_TVL1_ALL_BRICKS 4
int ojf_fuse_depth_hist(uint16_t *hist_dev /* fp16 [X,Y,Z,S] */, int n_bins, int X, int Y, int Z, const double *origin_host,
                        double resolution, int n, const double *K_host /* f64[n][9] */, const double *E_host /* f64[n][12] */,
                        const float *depth_dev /* f32[n,h,w] */, const uint8_t *mask_dev /* u8[n,h,w] or NULL */, int h, int w,
                        float trunc, float max_weight, float near, int carve, ojf_stream_t stream);
size_t ojf_tvl1_workspace_bytes(int X, int Y, int Z);
int ojf_tvl1_solve(const uint16_t *hist_dev, int n_bins, int X, int Y, int Z, float lambda, float tau, float sigma, int iterations,
                   int restart, float *u_dev /* f32 [X,Y,Z] */, void *workspace_dev, size_t workspace_bytes, ojf_stream_t stream);
int ojf_tvl1_write(const uint16_t *hist_dev, int n_bins, int X, int Y, int Z, const float *u_dev, float trunc,
                   uint16_t *tsdf_dev /* fp16 [X,Y,Z] */, uint16_t *weights_dev /* fp16 [X,Y,Z] */, ojf_stream_t stream);

/* ---- LABEL TV (the fused class distributions regularised in space: the convex relaxation of the Potts model on the label
 * volume; definition: csrc/ojf_label_tv.hip; the reference has no counterpart) -------------------------------
 * probs_dev is a label volume as ojf_fuse_label_probs makes it: fp16 [X,Y,Z,S], 16-byte aligned, S = 8 * ceil((C + 1) / 8),
 *   channels 0..C-1 = P_k, channel C = W (a voxel with W > 0 is observed), here with 2 <= C <= OJF_LABEL_TV_MAX_CLASSES.
 *   The solver minimises  sum_k TV(u_k) - lambda * sum_x omega(x) <u(x), P(x)>  over fields with u(x) in the simplex at
 *   every observed voxel, omega = min(W, w_sat) / w_sat; an edge between two 6-neighbours counts when both are observed and
 *   inside the box; unobserved voxels are never written and never influence an observed one.
 * The workspace (256-byte aligned, owned by one probs_dev and box between calls): a 256-byte header {u32 count of listed
 *   bricks, i32 status, ...}, then for the nb = ceil(X/4) * ceil(Y/8) * ceil(Z/32) bricks of 4 x 8 x 32 voxels, each part
 *   rounded up to 256 bytes: u32 [nb] (brick holds an observed voxel), i32 [nb] (brick -> slot, -1: not listed), u32 [nb]
 *   (slot -> brick), u8 [nb][1024] (voxel flags; bit 3: observed; voxel (lx, ly, lz) of a brick at (lx * 8 + ly) * 32 + lz),
 *   and then the state, f32 [capacity][C][1024] five times: u, ub, p_x, p_y, p_z - 20 * C * 1024 bytes per listed brick.
 * ojf_label_tv_workspace_bytes: the bytes for `capacity_bricks` slots; with 0, what ojf_label_tv_setup alone needs (and where
 *   the state begins: a larger workspace starts with the same bytes).  0 for what it refuses.
 * ojf_label_tv_setup: the set-up pass - flags, brick list, slot table - and the count of listed bricks into the header and
 *   into *count_dev (device memory), which is what the caller sizes the state by.  Two launches; never waits.
 * ojf_label_tv_solve: mode OJF_LABEL_TV_RESTART sets u = ub = the simplex projection of P and a zero dual on the listed
 *   bricks; OJF_LABEL_TV_CONTINUE goes on from the state the previous call with the same capacity left - N iterations in one
 *   call give the bits of any split of N over consecutive calls.  There is no refresh: when probs_dev took views, set up and
 *   restart.  lambda > 0, w_sat > 0, tau, sigma > 0 with tau * sigma <= 1/12, iterations >= 0.  *status_dev (device memory)
 *   and the header's status: 0 solved; 1 more bricks are listed than capacity_bricks - every kernel of the solve and of a
 *   following write does nothing; 2 there is no state to work on (no set-up pass on this workspace, a continue before any
 *   restart or with another capacity or class count).  One launch, one more for a restart, two per iteration; never waits.
 * ojf_label_tv_write: for every observed voxel ids_dev u8 [X,Y,Z] = the smallest k with the largest u_k, scores_dev fp16
 *   [X,Y,Z] = that u_k, and, if probs_out_dev is given (a record volume of the same C, 16-byte aligned; probs_dev itself is
 *   allowed), its channels k = u_k with W copied bit for bit and the padding untouched.  Every other voxel keeps what it holds.
 * Bad arguments (probs_dev off the 16-byte grid, n_classes outside 2..OJF_LABEL_TV_MAX_CLASSES, tau * sigma > 1/12,
 *   lambda <= 0, w_sat <= 0, negative iterations, a misaligned or short workspace) are refused before any HIP call.  The exact
 *   fp32 operation order is in csrc/ojf_label_tv.hip. */
#define OJF_LABEL_TV_MAX_CLASSES 32
#define OJF_LABEL_TV_CONTINUE 0
#define OJF_LABEL_TV_RESTART 1
size_t ojf_label_tv_workspace_bytes(int X, int Y, int Z, int n_classes, uint32_t capacity_bricks);
int ojf_label_tv_setup(const uint16_t *probs_dev /* fp16 [X,Y,Z,S] */, int n_classes, int X, int Y, int Z, void *workspace_dev,
                       size_t workspace_bytes, uint32_t *count_dev, ojf_stream_t stream);
int ojf_label_tv_solve(const uint16_t *probs_dev, int n_classes, int X, int Y, int Z, float lambda, float w_sat, float tau, float sigma,
                       int iterations, int mode, uint32_t capacity_bricks, void *workspace_dev, size_t workspace_bytes,
                       int32_t *status_dev, ojf_stream_t stream);
int ojf_label_tv_write(const uint16_t *probs_dev, int n_classes, int X, int Y, int Z, const void *workspace_dev, size_t workspace_bytes,
                       uint8_t *ids_dev /* u8 [X,Y,Z] */, uint16_t *scores_dev /* fp16 [X,Y,Z] */,
                       uint16_t *probs_out_dev /* fp16 [X,Y,Z,S] or NULL */, ojf_stream_t stream);

/* ---- FRAMES (the live depth frame made ready for tracking and fusion: edge rejection, bilateral filter, vertex / normal map;
 * definition: csrc/ojf_frames.hip; the reference only erodes its depth maps) ----------------------------------
 * ojf_depth_prepare: n frames depth_dev f32 [n,h,w] (with mask_dev u8 [n,h,w] or NULL) through, in this order,
 *   validity (finite, near <= d <= far, mask != 0; an invalid pixel counts as d = 0 and is never a neighbour),
 *   edge rejection (a valid pixel with a valid 8-neighbour further than edge_abs + edge_rel * d in depth is dropped; the test
 *     reads the validity of the first step, so nothing cascades; off when both thresholds are 0),
 *   a bilateral filter of radius 0..4 (0 copies) over the pixels that are left, with the spatial weights spatial_host f32
 *     [(2 * radius + 1)^2] (row-major window, values in 0..1, centre 1; NULL for radius 0) and the polynomial range kernel
 *     (1 - t^2)^2 for |t| < 1, t = (d_n - d) / (range0 + range2 * d^2),
 *   the camera-space vertex map V = ((c - cx) * ifx * f, (r - cy) * ify * f, f) of the filtered depth f and its unit normals
 *     (cross product of central differences, one-sided beside a pixel that is not valid; flipped to face the camera) - only
 *     when normals_out_dev is given or cos_min != 0 - with K_host f32 [n][4] = (1/fx, 1/fy, cx, cy) per frame,
 *   and an incidence test (a pixel without a normal, or whose normal makes a cosine below cos_min with the direction to the
 *     camera, is dropped; off when cos_min == 0).
 *   depth_out_dev f32 [n,h,w]: the filtered depth, 0 where the pixel is not valid - what every operator above reads as "no
 *   depth"; valid_out_dev u8 [n,h,w] (0 / 1) or NULL; normals_out_dev f32 [n,h,w,3] or NULL, 0 where the pixel is not valid
 *   or has no normal.  Every output element is written exactly once.
 * One launch for all stages (per 64 frames): a workgroup keeps a 32 x 8 pixel tile with its halo of at most radius + 2 in
 *   LDS from the raw frame to the outputs.  No global intermediate, no atomics, no workspace, never waits; the same bits on
 *   every run and for every split of the frames into calls.
 * Refused before any HIP call: null depth_dev / depth_out_dev; n, h, w < 1 or n * h * w >= 2^31; radius outside 0..4;
 *   radius > 0 without spatial_host, or with a weight outside 0..1 or a centre that is not 1; range0 <= 0, range2 < 0, a
 *   negative threshold, near < 0, far < near, cos_min outside 0..1, anything non-finite but far; K_host NULL with
 *   normals_out_dev or cos_min != 0; a float pointer off the 4-byte grid; an output that overlaps an input or another output
 *   (a tile reads its neighbours' pixels: there is no in-place operation).  The exact fp32 operation order is in
 *   csrc/ojf_frames.hip. */
int ojf_depth_prepare(const float *depth_dev /* f32[n,h,w] */, const uint8_t *mask_dev /* u8[n,h,w] or NULL */, int n, int h, int w,
                      const float *K_host /* f32[n][4] or NULL */, int radius, const float *spatial_host, float range0, float range2,
                      float edge_abs, float edge_rel, float near, float far, float cos_min, float *depth_out_dev,
                      uint8_t *valid_out_dev /* or NULL */, float *normals_out_dev /* f32[n,h,w,3] or NULL */, ojf_stream_t stream);

/* ---- RELOC (keyframe relocalisation by randomised ferns: a code per frame, a device store of keyframe codes and poses, the
 * nearest-keyframe search; definition: csrc/ojf_reloc.hip; the reference takes every pose from its dataset) ---
 * A frame's code: the frame is cut into cells of `cell` x `cell` pixels (1..64; CH = h / cell rows of CW = w / cell cells,
 *   trailing rows and columns ignored, CH * CW <= 1024); a cell's channel 0 is the mean of the depths of its valid pixels
 *   (mask != 0, finite, 0 < d < 64) quantised to 1/1024 m, valid when at least half of the pixels are, and channels 1..3 the
 *   means of the R, G, B bytes of image_dev (u8 [n,h,w,4], color.pack_image; without an image 0).  Fern m of n_ferns (a
 *   multiple of 8 in 8..4096) makes 4 bits "value(cell, channel) > threshold" from entries [m][0..3] of fern_cell_dev i32,
 *   fern_channel_dev u8 (0..3) and fern_threshold_dev f32 (device memory; a bit of channel 0 also needs a valid cell); its
 *   nibble sits in word m / 8 at bits 4 * (m % 8): n_ferns / 8 u32 words per frame.  Two codes differ by the number of
 *   ferns whose nibbles differ.
 * A store is device memory the caller owns: db_codes_dev u32 [capacity][n_ferns / 8], db_poses_dev f64 [capacity][12],
 *   db_count_dev i32 [1] (set it to 0 before the first insert).  The count is read and written on the device only.
 * ojf_reloc_encode: codes_dev u32 [n][n_ferns / 8] of n frames, and the code image f32 [n][4][CH][CW] if asked for (an
 *   invalid cell holds 0).  One launch, one workgroup per frame.
 * ojf_reloc_query: for each of n codes the k (1..16) smallest keys (u64) differ << 32 | keyframe over the first count
 *   keyframes, ascending (equal codes: smallest keyframe first); places beyond count hold all-ones.  One launch, or two and
 *   a stream-ordered scratch allocation for a capacity above 256.
 * ojf_reloc_insert: the n frames in call order - best_dev[i] = the smallest key over the store as it stands (all-ones when
 *   empty); the frame is wanted when force != 0, or the store is empty, or best's count > min_differ; added_dev[i] = 0 not
 *   wanted, 2 wanted but count == capacity (nothing is written), 1 added: code and pose copied to slot count, count + 1.
 *   One launch of one workgroup.
 * No float atomics, no workgroup waits for another, never waits; the same bits on every run and for every split of the
 *   frames into calls.  Refused before any HIP call: a null pointer other than mask_dev, image_dev, code_image_dev; n, h,
 *   w < 1 or n * h * w >= 2^31; cell outside 1..64 or larger than the frame, more than 1024 cells; n_ferns no multiple of 8
 *   in 8..4096; capacity outside 1..2^24; k outside 1..16; n > 65535 queries; min_differ outside 0..n_ferns; a pointer off
 *   the grid of its element type, fern_cell_dev / fern_threshold_dev off the 16-byte grid, fern_channel_dev off the 4-byte
 *   grid. */
int ojf_reloc_encode(const float *depth_dev /* f32[n,h,w] */, const uint8_t *mask_dev /* u8[n,h,w] or NULL */,
                     const uint8_t *image_dev /* u8[n,h,w,4] or NULL */, int n, int h, int w, int cell, int n_ferns,
                     const int32_t *fern_cell_dev /* i32[M][4] */, const uint8_t *fern_channel_dev /* u8[M][4] */,
                     const float *fern_threshold_dev /* f32[M][4] */, uint32_t *codes_dev /* u32[n][M/8] */,
                     float *code_image_dev /* NULL or f32[n][4][CH][CW] */, ojf_stream_t stream);
int ojf_reloc_query(const uint32_t *codes_dev /* u32[n][M/8] */, int n, int n_ferns, const uint32_t *db_codes_dev,
                    const int32_t *db_count_dev, int capacity, int k, uint64_t *keys_dev /* u64[n][k] */, ojf_stream_t stream);
int ojf_reloc_insert(const uint32_t *codes_dev /* u32[n][M/8] */, const double *poses_dev /* f64[n][12] */, int n, int n_ferns,
                     int min_differ, int force, uint32_t *db_codes_dev, double *db_poses_dev, int32_t *db_count_dev, int capacity,
                     uint64_t *best_dev /* u64[n] */, int32_t *added_dev /* i32[n] */, ojf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OJF_H */
