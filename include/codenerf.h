/*
 * codenerf.h -- C ABI of the MI355X (gfx950) CodeNeRF render/train hot path.
 *
 * The reference (yuliangguo/code-nerf) has no FFI: its hot path is a set of
 * Python calls made by both loops (src/trainer.py:65-84, src/optimizer.py:
 * 75-94).  Each entry point below replaces one of them; the comment names the
 * reference interface (file:line) it stands in for.
 *
 * Conventions
 *   - All buffers are DEVICE pointers owned by the caller (plain float32 unless
 *     stated), all sizes are element counts, every call is asynchronous on the
 *     given HIP stream (hipStream_t passed as void*; NULL = default stream).
 *   - Return 0 on success, a negative code on error; cn_last_error() gives a
 *     thread-local message.  No C++ exception crosses the ABI; no call
 *     allocates device memory (workspaces are caller-provided, sized by the
 *     cn_*_bytes queries).
 *   - Parameters are addressed through a device array of float* in the
 *     reference state_dict order (encoding_xyz.0.weight, encoding_xyz.0.bias,
 *     shape_latent_layer_1.0.weight, ... rgb.2.bias; src/model.py:20-34);
 *     gradients likewise (accumulated, like autograd's .grad).
 *   - Sample index m = ray * n_samples + s (reference layout (R, N, ...)).
 *     Per-sample outputs must be sized for cn_pad_samples(plan, M) samples.
 */
#ifndef CODENERF_H
#define CODENERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CN_ABI_VERSION 4
#define CN_FP32 0 /* exact-fp32 MFMA path (parity) */
#define CN_BF16 1 /* bf16 operands, fp32 accumulate (throughput) */
/* error-compensated bf16: weights and chain operands as bf16 hi + lo pairs,
 * three MFMAs per block into fp32 (~16-bit operands); dW as CN_BF16 */
#define CN_BF16X3 2
/* the CN_BF16X3 forward chains (rendered rgb at fp32 class) with the CN_BF16
 * backward (dX chain and dW on bf16 operands); the training forward stores the
 * CN_BF16 planes (hi parts only) */
#define CN_BF16X3F 3
/* Largest sample count (M, act_M, R * N) one call accepts: the kernels index
 * samples with 32-bit integers (3 m, 4 m).  Larger images are rendered in
 * ray parts (codenerf_amd.render.ImageStep / CodeNeRF.forward split
 * automatically); a call above the limit returns -1 with cn_last_error().
 * The activation planes have no 4 GB limit: every wave addresses its own
 * 32-sample slab through a 64-bit descriptor base. */
#define CN_MAX_SAMPLES (1 << 28)

typedef struct cn_plan cn_plan;

int cn_abi_version(void);
const char *cn_last_error(void);

/* Measurement hook (no reference counterpart; ABI 3): the next chain, dW or
 * bias-sum kernel the calling thread launches records start_event /
 * stop_event (hipEvent_t, created by the caller) from its own dispatch
 * packet (hipExtLaunchKernel), so a per-kernel timer adds no marker packets
 * between kernels.  Give both or neither (NULL, NULL clears). */
int cn_time_next_launch(void *start_event, void *stop_event);

/* Stream dependency on one device (ABI 3): `waiter` waits for the work queued
 * so far on `signaller`, through an event WITHOUT the system-scope fence a
 * default event record performs (an L2 write-back of everything the last
 * kernel dirtied: ~15 us behind a chain or dW launch).  For the dX / dW
 * pipelining of one step (render.ImageStep); host-visible results still need
 * the stream's own synchronisation. */
int cn_stream_wait(void *waiter_stream, void *signaller_stream);

/* Clock probe (measurement only, no reference counterpart): n_workgroups
 * workgroups of 4 waves issue `iters` x 4 back-to-back bf16 MFMAs
 * (v_mfma_f32_32x32x16_bf16) on hashed operands; wave 0 of each stamps the
 * shader-cycle counter and the 100 MHz real-time counter around the loop:
 * d_out[3 g + 0] = cycles, [3 g + 1] = 100 MHz ticks, [3 g + 2] = a checksum.
 * Effective clock = cycles / ticks x 100 MHz (bench.py records it beside a
 * step time, so box-to-box clock differences can be told from regressions). */
int cn_clock_probe(unsigned int *d_out, int n_workgroups, int iters, unsigned int seed, void *stream);

/* ---- plan: static layout for one network configuration and precision.
 * Replaces CodeNeRF.__init__ (src/model.py:11-34).  Creating a plan and the
 * size queries need no device (tables go up with the first cn_pack_weights).
 * Supported:
 * W = latent_dim = 256, num_xyz_freq = 10, num_dir_freq = 4,
 * (shape_blocks, texture_blocks) in {(3,1), (2,1)}. */
int cn_plan_create(int shape_blocks, int texture_blocks, int W, int num_xyz_freq,
                   int num_dir_freq, int latent_dim, int precision, cn_plan **out);
void cn_plan_destroy(cn_plan *plan);
int cn_plan_num_params(const cn_plan *plan);        /* tensors in the state_dict */
int cn_plan_num_inject(const cn_plan *plan);        /* shape + texture blocks */
int cn_pad_samples(const cn_plan *plan, int M);     /* M rounded to the tile (-1: M invalid) */
int cn_max_samples(void);                           /* CN_MAX_SAMPLES */
size_t cn_act_bytes_per_sample(const cn_plan *plan); /* workspace bytes per sample (splitting) */
size_t cn_packed_bytes(const cn_plan *plan, int bwd); /* packed weights */
size_t cn_blob_floats(const cn_plan *plan);         /* per-call bias blob */
size_t cn_act_bytes(const cn_plan *plan, int M);    /* training activations */
size_t cn_dw_ws_bytes(const cn_plan *plan, int M);  /* weight-grad partials */
/* Layout introspection of the training workspace laid out for M samples
 * (tests and debugging): byte offset of a plane (-1 if it does not exist);
 * *width = its elements per sample (masks: bytes per sample).  Plane
 * element layout: code-nerf_amd/csrc/cn_layout.h (slab_off / plane_off). */
#define CN_PLANE_Y 0     /* index: forward layer whose output it is */
#define CN_PLANE_DA 1    /* index: forward layer whose pre-activation gradient it is */
#define CN_PLANE_PE 2
#define CN_PLANE_DIR 3
#define CN_PLANE_MASKS 4
/* bf16x3 plans only (-1 otherwise): the lo parts rn(x - rn(x)) of the dW
 * pass's X operands, stored by the training forward beside the hi planes */
#define CN_PLANE_YLO 5   /* index: forward layer whose output it is */
#define CN_PLANE_PELO 6
long long cn_act_plane(const cn_plan *plan, int M, int kind, int index, int *width);

/* ---- weights: pack the parameters into the chain kernels' fragment order
 * (fwd: W, bwd: W^T).  Call after every optimiser step. */
int cn_pack_weights(const cn_plan *plan, const float *const *d_params, void *d_pack_fwd,
                    void *d_pack_bwd, void *stream);

/* ---- per-object latent layers, src/model.py:41,49: z_j = ReLU(L_j c + c_j),
 * folded into the next layer's bias (b + W z).  d_blob: cn_blob_floats floats,
 * d_zvec: num_inject x 256. */
int cn_latent_fwd(const cn_plan *plan, const float *const *d_params, const float *d_shape_code,
                  const float *d_texture_code, float *d_blob, float *d_zvec, void *stream);

/* ---- CodeNeRF.forward (src/model.py:36-53) for M samples.
 * mode A (d_xyz != NULL): explicit points xyz/viewdir [M][3];
 * mode B (d_xyz == NULL): samples of rays, xyz = rays_o + rays_d * z
 *   (src/utils.py:30), z = d_z[ray * z_stride + s] (z_stride 0: one z vector
 *   shared by all rays as in the reference, n_samples: per-ray z).
 * d_sigma [Mp], d_rgb [Mp][3].  d_act != NULL stores what the backward
 * needs: the workspace holds cn_act_bytes(plan, act_M) bytes (act_M <= 0:
 * act_M = M) and this call fills its sample rows [act_row0, act_row0 + Mp)
 * (act_row0 a multiple of cn_pad_samples' granule, 256), so the coarse and
 * the fine pass of one image share one workspace and one backward. */
int cn_mlp_fwd(const cn_plan *plan, const void *d_pack_fwd, const float *d_blob, int M,
               const float *d_xyz, const float *d_viewdir, const float *d_rays_o,
               const float *d_rays_d, const float *d_z, int z_stride, int n_samples,
               float *d_sigma, float *d_rgb, void *d_act, int act_M, int act_row0,
               void *stream);

/* ---- autograd of CodeNeRF.forward (src/trainer.py:82): dX chain. */
int cn_mlp_bwd(const cn_plan *plan, const void *d_pack_bwd, const float *d_blob, int M,
               const float *d_dsigma, const float *d_drgb, void *d_act, void *stream);

/* ---- the same over rows [act_row0, act_row0 + pad(M)) of a workspace laid
 * out for act_M samples (act_row0 a multiple of 256); d_dsigma / d_drgb point
 * at the range's first row.  The coarse and fine rows of one training step
 * (src/trainer.py:82 over both passes) are back-propagated by two launches so
 * the weight gradients of the first range (cn_mlp_dw_rows, on a second
 * stream) overlap the dX chain of the second. */
int cn_mlp_bwd_rows(const cn_plan *plan, const void *d_pack_bwd, const float *d_blob, int M,
                    const float *d_dsigma, const float *d_drgb, void *d_act, int act_M, int act_row0,
                    void *stream);

/* ---- codes-only optimisation (src/optimizer.py:75-98: the model is fixed,
 * only the latent codes are updated).  Same arguments as cn_mlp_fwd /
 * cn_mlp_bwd_rows (d_act required); the forward stores only what the backward
 * needs (ReLU masks, sigma pre-activations), the backward only the gradient
 * planes of the layers fed by a code -- what cn_mlp_dbias reads -- and none of
 * the weight-gradient operands. */
int cn_mlp_fwd_codes(const cn_plan *plan, const void *d_pack_fwd, const float *d_blob, int M,
                     const float *d_xyz, const float *d_viewdir, const float *d_rays_o,
                     const float *d_rays_d, const float *d_z, int z_stride, int n_samples,
                     float *d_sigma, float *d_rgb, void *d_act, int act_M, int act_row0,
                     void *stream);
int cn_mlp_bwd_codes(const cn_plan *plan, const void *d_pack_bwd, const float *d_blob, int M,
                     const float *d_dsigma, const float *d_drgb, void *d_act, int act_M,
                     int act_row0, void *stream);

/* ---- camera-pose refinement (no reference counterpart; ABI 4: the reference
 * lists "Pose Optimizing" as not done).  cn_mlp_bwd_pose: the backward of a
 * cn_mlp_fwd_codes forward, same arguments as cn_mlp_bwd_codes; it stores what
 * that call stores plus the two input-side gradient planes cn_mlp_input_grad
 * reads (dA of encoding_xyz and of encoding_viewdir).  The training backward
 * (cn_mlp_bwd / cn_mlp_bwd_rows) stores both planes too. */
int cn_mlp_bwd_pose(const cn_plan *plan, const void *d_pack_bwd, const float *d_blob, int M,
                    const float *d_dsigma, const float *d_drgb, void *d_act, int act_M,
                    int act_row0, void *stream);

/* ---- gradient with respect to the network inputs (no reference counterpart;
 * the autograd of src/model.py:4-7,38,47 restated), for rows [act_row0,
 * act_row0 + pad(M)) of a workspace laid out for act_M samples (act_M <= 0: M)
 * after cn_mlp_bwd_pose or cn_mlp_bwd_rows over the same rows.  The inputs are
 * those of the forward: mode A (d_xyz != NULL) or mode B exactly as cn_mlp_fwd
 * selects them.  d_params: the parameter tensors the forward used.
 * d_dxyz, d_dviewdir [Mp][3] are written (rows >= M as 0); -grad sigma of a
 * sample is its surface normal.  Mode B, optional (both or none; NULL in mode
 * A): d_drays_o [R][3] = sum_s d_xyz and d_drays_d [R][3] = sum_s (z_s d_xyz +
 * d_viewdir) over each ray's n_samples rows, summed in float64 in a fixed
 * order (deterministic, written).  Returns -1 with cn_last_error() for rows
 * outside the workspace or act_row0 not a multiple of 256. */
int cn_mlp_input_grad(const cn_plan *plan, const float *const *d_params, const void *d_act,
                      int act_M, int act_row0, int M, const float *d_xyz,
                      const float *d_viewdir, const float *d_rays_o, const float *d_rays_d,
                      const float *d_z, int z_stride, int n_samples, float *d_dxyz,
                      float *d_dviewdir, float *d_drays_o, float *d_drays_d, void *stream);

/* ---- weight / bias gradients, accumulated into d_grads; d_dbuf
 * (num_inject x 256) receives this call's bias gradient of every layer fed by
 * a latent code (input of cn_latent_bwd).  d_params: the parameter tensors the
 * forward used (the table given to cn_pack_weights): encoding_shape's planes
 * are not stored, its gradients and those of the layers reading its output
 * (sigma head, encoding_viewdir) are folded through its weights. */
int cn_mlp_dw(const cn_plan *plan, void *d_act, int M, const float *d_zvec,
              const float *const *d_params, float *const *d_grads, float *d_dbuf, void *d_ws,
              void *stream);

/* ---- cn_mlp_dw over rows [act_row0, act_row0 + pad(M)) of a workspace laid
 * out for act_M samples (act_row0 a multiple of 256).  db_accum != 0 adds
 * this range's bias gradients into d_dbuf instead of overwriting it (the
 * later ranges of a step).  Grads accumulate as in cn_mlp_dw.
 * n_workgroups: persistent workgroups of the pass (0 = one per CU, 256);
 * fewer leave CUs to a dX chain running beside it on another stream (at
 * least 26: a workgroup's share must not span more than two layers). */
int cn_mlp_dw_rows(const cn_plan *plan, void *d_act, int act_M, int act_row0, int M,
                   const float *d_zvec, const float *const *d_params, float *const *d_grads,
                   float *d_dbuf, int db_accum, int n_workgroups, void *d_ws, void *stream);

/* ---- bias gradients of the layers after each code injection only (d_dbuf
 * [n_inject][256], as cn_mlp_dw writes them), for codes-only optimisation
 * (src/optimizer.py:92: the model is fixed, only the codes are updated, so
 * no weight gradients are needed), over rows [0, pad(M)) of a workspace laid
 * out for act_M samples (act_M <= 0: M).  d_ws: cn_dw_ws_bytes(plan, M) bytes. */
int cn_mlp_dbias(const cn_plan *plan, void *d_act, int act_M, int M, float *d_dbuf, void *d_ws,
                 void *stream);

/* ---- latent layers + code gradients (+ the code regulariser of
 * src/trainer.py:76-78 when reg_coef != 0; *d_reg_out = reg value:
 * written, not accumulated; 0 when reg_coef == 0).
 * d_scratch: num_inject x 256 floats.  d_dshape / d_dtex accumulate. */
int cn_latent_bwd(const cn_plan *plan, const float *const *d_params, float *const *d_grads,
                  const float *d_shape_code, const float *d_texture_code, const float *d_zvec,
                  const float *d_dbuf, float *d_scratch, float *d_dshape, float *d_dtex,
                  float reg_coef, float *d_reg_out, void *stream);

/* ---- geometry / rendering --------------------------------------------- */
/* get_rays, src/utils.py:10-19.  d_c2w: 4x4 row-major.  focal_is_f64: the
 * reference receives focal as a float64 tensor from default_collate and forms
 * the camera directions in float64 (type promotion) before casting. */
int cn_get_rays(int H, int W, double focal, int focal_is_f64, const float *d_c2w,
                float *d_rays_o, float *d_viewdirs, void *stream);
/* autograd of get_rays with respect to c2w (no reference counterpart; ABI 4).
 * Same (H, W, focal, focal_is_f64, d_c2w) as the forward, plus the gradients
 * of its outputs [H*W][3]; d_dc2w: 12 floats (3x4 row-major: rotation columns,
 * then translation), written, not accumulated.  Two-stage float64 sum in a
 * fixed order (deterministic).  d_ws: cn_get_rays_bwd_ws_bytes(H, W) bytes
 * (0: H, W invalid). */
size_t cn_get_rays_bwd_ws_bytes(int H, int W);
int cn_get_rays_bwd(int H, int W, double focal, int focal_is_f64, const float *d_c2w,
                    const float *d_drays_o, const float *d_dviewdirs, float *d_dc2w, void *d_ws,
                    void *stream);
/* sample_from_rays point expansion, src/utils.py:30-31 */
int cn_sample_points(const float *d_rays_o, const float *d_viewdirs, const float *d_z, int z_stride,
                     int R, int N, float *d_xyz, float *d_viewdir_rep, void *stream);
/* volume_rendering, src/utils.py:34-47 (N <= 256).  d_weights may be NULL. */
int cn_composite_fwd(const float *d_sigma, const float *d_rgb, const float *d_z, int z_stride,
                     int R, int N, int white_bg, float *d_out_rgb, float *d_out_depth,
                     float *d_weights, void *stream);
/* autograd of volume_rendering; d_grad_depth may be NULL */
int cn_composite_bwd(const float *d_sigma, const float *d_rgb, const float *d_z, int z_stride,
                     int R, int N, int white_bg, const float *d_grad_rgb,
                     const float *d_grad_depth, float *d_dsigma, float *d_drgb, void *stream);
/* training: composite + chunk-mean MSE (src/trainer.py:69,75; chunk = batch
 * size B) + its gradient w.r.t. sigma / rgb.  d_chunk_loss: ceil(R/chunk). */
int cn_render_loss(const float *d_sigma, const float *d_rgb, const float *d_z, int z_stride,
                   int R, int N, int white_bg, const float *d_gt, int chunk, float *d_out_rgb,
                   float *d_ray_se, float *d_chunk_loss, float *d_dsigma, float *d_drgb,
                   void *stream);

/* ---- hierarchical sampling (BASELINE configs' "64 coarse + 64 fine"; the
 * reference has no fine pass -- NeRF's sample_pdf restated, oracle
 * oracle/ref_cpu.py:sample_pdf).  Per ray: bins = midpoints of the coarse z,
 * pdf = weights[1:-1] + 1e-5 normalised, u_j = (j + d_rand[ray][j]) / Nf,
 * d_z_f [R][Nf] = inverse cdf (ascending). */
int cn_sample_pdf(const float *d_sigma_c, const float *d_z_c, int zc_stride, int R, int Nc,
                  const float *d_rand, int Nf, float *d_z_f, void *stream);

/* fine composite over the union of each ray's coarse and fine samples
 * (merged by z) + chunk-mean MSE + backward.  d_dsig_c / d_drgb_c are
 * accumulated into (they hold the coarse loss's gradient from
 * cn_render_loss); d_dsig_f / d_drgb_f [R*Nf] are written. */
int cn_render_loss_fine(const float *d_sigma_c, const float *d_rgb_c, const float *d_z_c,
                        int zc_stride, int Nc, const float *d_sigma_f, const float *d_rgb_f,
                        const float *d_z_f, int Nf, int R, int white_bg, const float *d_gt,
                        int chunk, float *d_out_rgb, float *d_ray_se, float *d_chunk_loss,
                        float *d_dsig_c, float *d_drgb_c, float *d_dsig_f, float *d_drgb_f,
                        void *stream);

/* ---- masked image loss (no reference counterpart in code; the paper's
 * real-image experiments mask the loss; additive to ABI 4).  The two loss
 * entries above with a weight m_r >= 0 per ray and a silhouette term on the
 * ray's accumulated opacity acc_r = sum_k w_k (over the merged samples in the
 * fine entry): per chunk of nb rays
 *   loss = sum_r [ m_r sum_c (col_rc - gt_rc)^2 + 3 sil_coef (acc_r - a_r)^2 ] / (3 nb)
 * (the denominator is the chunk's size, not sum m: defined for a chunk
 * without foreground), d_ray_se[r] holding the bracket.  Arguments as the
 * plain entry's, then: d_ray_weight [R] (NULL: m = 1), d_acc_target [R] = a
 * (NULL: no silhouette term), sil_coef >= 0 (0: no silhouette term),
 * d_out_acc [R] = acc, may be NULL.  m = 1 and no silhouette term give the
 * plain entry's results bit for bit.  Returns -1 with cn_last_error() before
 * any launch for the plain entry's refusals, a z stride other than 0 or the
 * coarse sample count, sil_coef negative or not finite, and sil_coef > 0
 * with a NULL d_acc_target. */
int cn_render_loss_masked(const float *d_sigma, const float *d_rgb, const float *d_z, int z_stride,
                          int R, int N, int white_bg, const float *d_gt, int chunk,
                          float *d_out_rgb, float *d_ray_se, float *d_chunk_loss, float *d_dsigma,
                          float *d_drgb, const float *d_ray_weight, const float *d_acc_target,
                          float sil_coef, float *d_out_acc, void *stream);
int cn_render_loss_fine_masked(const float *d_sigma_c, const float *d_rgb_c, const float *d_z_c,
                               int zc_stride, int Nc, const float *d_sigma_f, const float *d_rgb_f,
                               const float *d_z_f, int Nf, int R, int white_bg, const float *d_gt,
                               int chunk, float *d_out_rgb, float *d_ray_se, float *d_chunk_loss,
                               float *d_dsig_c, float *d_drgb_c, float *d_dsig_f, float *d_drgb_f,
                               const float *d_ray_weight, const float *d_acc_target, float sil_coef,
                               float *d_out_acc, void *stream);

/* forward half of cn_render_loss_fine (test-time rendering; additive to ABI
 * 4): the same merge of each ray's coarse and fine samples (a coarse sample
 * precedes a fine one at equal z; Nc + Nf <= 256, zc_stride 0 or Nc), so
 * d_out_rgb [R][3] equals that call's bit for bit; d_out_depth [R] = sum w z
 * over the merged samples; d_out_acc [R] = sum w, may be NULL. */
int cn_composite_fine_fwd(const float *d_sigma_c, const float *d_rgb_c, const float *d_z_c,
                          int zc_stride, int Nc, const float *d_sigma_f, const float *d_rgb_f,
                          const float *d_z_f, int Nf, int R, int white_bg, float *d_out_rgb,
                          float *d_out_depth, float *d_out_acc, void *stream);

/* ---- geometry buffers of a composited ray (additive to ABI 4; no reference
 * counterpart).  cn_composite_fwd (Nf == 0, the three fine
 * pointers and d_grad_f NULL) or cn_composite_fine_fwd (Nf > 0, the same merge)
 * with two more outputs.  Over the ray's (merged) samples k = 0 .. N-1 with
 * the compositing weights w_k:
 *   d_out_rgb [R][3], d_out_depth [R], d_out_acc [R] (may be NULL): those
 *     entries' rgb, depth = sum w z and weight sum, bit for bit;
 *   d_out_depth_med [R] (may be NULL): z_m of the first sample m with C_m >=
 *     0.5, C_k the running float64 sum of w_j, j <= k, in sample order; z_{N-1}
 *     when the ray never gets there (the closing interval puts the leftover
 *     transmittance at the last sample, so only non-finite weights do that);
 *   d_out_normal [R][3] (may be NULL): sum_k w_k u_k, NOT normalised (its
 *     length is at most acc and says how much surface the ray met), with u_k =
 *     -g_k / |g_k| in float32 and (0, 0, 0) unless |g_k| > 0; g = d sigma / d
 *     xyz per sample, d_grad_c [R*Nc][3] and d_grad_f [R*Nf][3] (what
 *     cn_mlp_bwd_pose with d sigma = 1, d rgb = 0 and cn_mlp_input_grad leave
 *     in d_dxyz).  Products rounded to float32, summed in float64 in a fixed
 *     order, rounded once.
 * No atomics; every output is deterministic and independent of which optional
 * pointers are NULL.  Returns -1 with a message starting "cn_composite_aov:",
 * before any launch, for: a NULL required pointer; Nc < 1 or Nf < 0; Nc + Nf >
 * 256; zc_stride other than 0 or Nc; Nf > 0 with a NULL fine pointer; Nf == 0
 * with a fine pointer given; d_out_normal without d_grad_c (and d_grad_f when
 * Nf > 0); a gradient pointer without d_out_normal; R < 1 or R * (Nc + Nf) >
 * CN_MAX_SAMPLES. */
int cn_composite_aov(const float *d_sigma_c, const float *d_rgb_c, const float *d_z_c, int zc_stride,
                     int Nc, const float *d_grad_c, const float *d_sigma_f, const float *d_rgb_f,
                     const float *d_z_f, int Nf, const float *d_grad_f, int R, int white_bg,
                     float *d_out_rgb, float *d_out_depth, float *d_out_acc,
                     float *d_out_depth_med, float *d_out_normal, void *stream);

/* ---- rendering through an occupancy grid (additive to ABI 4; no reference
 * counterpart).  The grid is G^3 cells (G a multiple of 32 in [32, 256]) over
 * the box [lo, lo + G / inv_cell)^3, one bit per cell: cell c = (ix G + iy) G
 * + iz is bit c & 31 of word c >> 5 of d_bits [G^3 / 32].  A sample s of ray r
 * is KEPT when its point, in float32 with separately rounded operations as
 * cn_mlp_fwd's ray mode forms it,
 *   x_a = o_a + d_a z,  t_a = (x_a - lo_a) inv_cell,  0 <= t_a < G (NaN: no),
 * lies in a set cell i_a = floor(t_a); with keep_last the last sample of every
 * ray is kept as well.  The sparse render of a view is the dense render with
 * the density and colour of every sample that is not kept replaced by 0: mark
 * -> exclusive prefix sum of d_count (the caller's) -> gather -> cn_mlp_fwd on
 * the explicit points -> scatter -> the unchanged compositing entries.  No
 * atomics: every output is deterministic.
 * Each entry returns -1 with cn_last_error() naming it, before any device
 * call, for a NULL pointer, R < 1, N outside [1, 256], R * N >
 * CN_MAX_SAMPLES, z_stride other than 0 or N, G not a multiple of 32 in
 * [32, 256], dilate outside [0, 4], tau NaN, inv_cell not finite and positive
 * or a lo that is not finite.
 *
 * cn_occupancy_build: d_sigma [G^3] holds the density at the cell centres in
 * the cell order above; a cell is occupied when sigma >= tau (NaN: occupied),
 * and its bit is the OR over the cells within Chebyshev distance `dilate`,
 * clamped at the box faces.  Every word of d_bits is written. */
int cn_occupancy_build(const float *d_sigma, int G, float tau, int dilate, uint32_t *d_bits,
                       void *stream);
/* d_keep [R][8]: bit s & 31 of word s >> 5 says sample s is kept (bits >= N and
 * unused words 0); d_count [R]: kept samples of the ray.  Both written. */
int cn_sparse_mark(const float *d_rays_o, const float *d_rays_d, const float *d_z, int z_stride,
                   int R, int N, const uint32_t *d_bits, int G, float lo_x, float lo_y, float lo_z,
                   float inv_cell, int keep_last, uint32_t *d_keep, int *d_count, void *stream);
/* d_offset [R]: the exclusive prefix sum of d_count.  Kept sample s of ray r
 * goes to row d_offset[r] + (kept samples of r below s) of d_xyz / d_viewdir
 * [Mk][3] (ray-major, samples ascending; Mk = sum of d_count): the point x
 * above and the ray direction.  Rows >= Mk are not written. */
int cn_sparse_gather(const float *d_rays_o, const float *d_rays_d, const float *d_z, int z_stride,
                     int R, int N, const uint32_t *d_keep, const int *d_offset, float *d_xyz,
                     float *d_viewdir, void *stream);
/* the inverse: d_sigma [R*N] and d_rgb [R*N][3] get the compact row at kept
 * samples and 0 elsewhere; every element is written. */
int cn_sparse_scatter(const uint32_t *d_keep, const int *d_offset, int R, int N,
                      const float *d_sigma_k, const float *d_rgb_k, float *d_sigma, float *d_rgb,
                      void *stream);

/* ---- several objects in one scene (additive to ABI 4; no reference
 * counterpart).  A scene is K objects, 1 <= K <= 8; object k has
 * its own codes and occupancy grid and a similarity transform from its frame to
 * the world: rotation R_k, translation t_k, scale s_k > 0.  Its field is
 * evaluated on the world ray seen from its frame, at the sample depths z / s_k,
 * through mark (keep_last 0) -> gather -> cn_mlp_fwd -> scatter; outside the
 * set cells of its grid its density and colour are 0.  With a_k = sigma_k / s_k
 * (the opacity sigma * delta does not depend on the scale) the scene's sample is
 *   sigma = sum_k a_k,  f_k = a_k / sigma (0 unless sigma > 0),
 *   rgb = sum_k f_k rgb_k,
 * composited as one object's.  Every float32 operation of the three entries is
 * rounded separately, in the order given; the division is correctly rounded.
 * No atomics: every output element is written by one lane.  The host arrays
 * (h_*) are read at the call.  Each entry returns -1 with a message starting
 * with its name, before any launch, for a NULL required pointer, K outside
 * [1, 8], a 1/s that is not finite and positive, or a size above
 * CN_MAX_SAMPLES, and for what its own comment lists.
 *
 * cn_scene_rays: h_xf [K][13] = R_k row-major (9), t_k (3), 1 / s_k, all
 * finite.  d_out_o, d_out_d [K][R][3], with q = o - t:
 *   o_k,a = ((R_0a q_0 + R_1a q_1) + R_2a q_2) * (1 / s_k)
 *   d_k,a = (R_0a d_0 + R_1a d_1) + R_2a d_2        (not re-normalised)
 * i.e. R^T (o - t) / s and R^T d; the identity with s = 1 hands o and d back
 * unchanged up to the sign of a zero.  Also refused: R < 1. */
int cn_scene_rays(const float *d_rays_o, const float *d_rays_d, int R, const float *h_xf, int K,
                  float *d_out_o, float *d_out_d, void *stream);
/* d_sigma_k [K][M], d_rgb_k [K][M][3], h_inv_s [K] = 1 / s_k -> d_sigma [M],
 * d_rgb [M][3] by the rule above, a_k = sigma_k * (1 / s_k), both sums left to
 * right over k starting from the first term; rgb is 0 unless sigma > 0 (a NaN
 * sum included).  With K = 1 and s = 1 the outputs are the inputs bit for bit
 * wherever sigma > 0.  Also refused: M < 1. */
int cn_scene_combine(const float *d_sigma_k, const float *d_rgb_k, const float *h_inv_s, int K,
                     int M, float *d_sigma, float *d_rgb, void *stream);
/* cn_composite_fwd (Nf == 0, every fine pointer NULL) or cn_composite_fine_fwd
 * on the combined planes, bit for bit: d_out_rgb [R][3], d_out_depth [R],
 * d_out_acc [R] (all required).  With the compositing weights w_i of the ray's
 * (merged) samples:
 *   d_obj_acc [R][K]: sum_i w_i f_k,i, with f_k,i formed as cn_scene_combine
 *     forms it from the object planes d_obj_c [K][R*Nc] / d_obj_f [K][R*Nf]
 *     (what went into cn_scene_combine) and the combined density; the products
 *     rounded to float32, summed in float64 in a fixed order, rounded once.
 *     The columns sum to d_out_acc up to rounding;
 *   d_instance [R] int32: the lowest k with the largest d_obj_acc[r][k] when
 *     d_out_acc[r] >= acc_min, else -1.
 * d_obj_acc and d_instance may be NULL together; the object planes are then
 * not read and may be NULL.  The three required outputs do not depend on that.
 * Also refused: Nc < 1, Nf < 0, Nc + Nf > 256, zc_stride other than 0 or Nc,
 * Nf > 0 with a NULL fine pointer, Nf == 0 with a fine pointer given, only one
 * of d_obj_acc / d_instance, labels without d_obj_c (and d_obj_f when Nf > 0),
 * acc_min NaN, R < 1 or R * (Nc + Nf) > CN_MAX_SAMPLES. */
int cn_scene_composite(const float *d_sigma_c, const float *d_rgb_c, const float *d_z_c,
                       int zc_stride, int Nc, const float *d_sigma_f, const float *d_rgb_f,
                       const float *d_z_f, int Nf, const float *d_obj_c, const float *d_obj_f,
                       const float *h_inv_s, int K, int R, int white_bg, float acc_min,
                       float *d_out_rgb, float *d_out_depth, float *d_out_acc, float *d_obj_acc,
                       int *d_instance, void *stream);

/* ---- iso-surface of a density lattice (additive to ABI 4; no reference
 * counterpart): marching tetrahedra on the Kuhn (Freudenthal) triangulation,
 * which has no ambiguous case, and whose face diagonals agree between
 * neighbouring cubes, so the surface is closed wherever the field is outside
 * on the lattice boundary.  DESIGN.md 8.5.
 * Lattice: nx x ny x nz points, point (ix, iy, iz) is c = (ix ny + iy) nz + iz
 * of d_field [P], P = nx ny nz.  A point is INSIDE iff !(field[c] < iso) (NaN:
 * inside); its position is p_a = lo_a + float(i_a) s_a per axis, in float32
 * with separately rounded operations.
 * Edges: point p owns edge k = 0..6 towards p + e_k, e_k = ((m >> 2) & 1,
 * (m >> 1) & 1, m & 1) with m = k + 1, when p + e_k is in the lattice.  An
 * edge CROSSES when exactly one end is inside; d_vflags[c] has bit k set for a
 * crossing owned edge and d_vcount[c] = popcount.  Each crossing edge carries
 * one vertex, row voff[c] + popcount(vflags[c] & ((1 << k) - 1)), voff the
 * exclusive prefix sum of vcount.  With a = p, b = p + e_k:
 *   t = (iso - s_a) / (s_b - s_a)   (correctly rounded; NaN -> 0.5; clamped to
 *   [0, 1]),   x = P_a + t (P_b - P_a)   per axis, separately rounded.
 * Tetrahedra: the cube with lowest corner p (ix < nx - 1, iy < ny - 1, iz <
 * nz - 1) is cut into 6, one per permutation pi of the axes (x, y, z) in
 * lexicographic order: v0 = p, v1 = v0 + axis pi0, v2 = v1 + axis pi1, v3 = p +
 * (1, 1, 1); edge (v_i, v_j), i < j, is an owned edge of v_i.  With the inside
 * corners `ins` and the outside ones `out` ascending: 1 inside (a): the
 * triangle [(a, o) for o in out]; 3 inside (o outside): [(i, o) for i in ins];
 * 2 inside (a < b; c < d outside): [(a,c), (a,d), (b,d)] then [(a,c), (b,d),
 * (b,c)].  Orientation, decided in the unit cube with every crossing at its
 * edge's midpoint: with g = mean of the outside corners - mean of the inside
 * corners, a triangle with ((q1 - q0) x (q2 - q0)) . g < 0 has its last two
 * entries swapped, so normals point from inside to outside (towards lower
 * density).  csrc/mesh_tables.h holds the resulting table, generated by
 * tools/gen_mesh_tables.py.
 * d_tcount[c]: triangles of the cube at c (at most 12; 0 where there is no
 * cube).  The cube's triangles are rows toff[c] ... of d_tri, toff the
 * exclusive prefix sum of tcount, in tetrahedron order, then in the order
 * above; a row holds three vertex rows.  No atomics: every output element is
 * written by exactly one thread.  The prefix sums are the caller's.
 * Both entries return -1 with cn_last_error() naming the entry, before any
 * device call, for a NULL pointer, a dimension outside [2, 1024], P > 2^27 (so
 * that 7 P and 12 P fit an int32), iso NaN, a spacing that is not finite and
 * positive, or a lo that is not finite.
 *
 * cn_mesh_count: d_vflags, d_vcount, d_tcount [P], every element written. */
int cn_mesh_count(const float *d_field, int nx, int ny, int nz, float iso, uint8_t *d_vflags,
                  int *d_vcount, int *d_tcount, void *stream);
/* d_vflags as cn_mesh_count left it for the same field and iso; d_voff, d_toff
 * [P] the exclusive prefix sums.  d_vert [Nv][3], d_tri [Nt][3] (Nv, Nt the
 * totals): rows >= Nv of d_vert and rows >= Nt of d_tri are not written. */
int cn_mesh_emit(const float *d_field, int nx, int ny, int nz, float iso, float lo_x, float lo_y,
                 float lo_z, float s_x, float s_y, float s_z, const uint8_t *d_vflags,
                 const int *d_voff, const int *d_toff, float *d_vert, int *d_tri, void *stream);

/* ---- evaluation metrics of the test-time loop (additive to ABI 4) for V
 * views at once: the PSNR argument of src/optimizer.py:117-125 and SSIM as
 * src/optimizer.py:156 calls it (skimage structural_similarity(multichannel=
 * True); codenerf_amd.metrics.ssim_legacy is the definition: 7x7 uniform
 * window, sample covariance, data_range 2, image cropped by 3 per side).
 * d_img, d_gt [V][H*W][3] contiguous, pixel = row * W + col (cn_get_rays'
 * order).  d_out [V][2] float64 = (mse, ssim) per view, written.  mse: per
 * chunk of `chunk` consecutive rays (ragged last chunk) the mean of
 * (img - gt)^2 over its 3 n elements, then the plain mean of the chunk means;
 * d_chunk_mse [V][ceil(H*W/chunk)] float64 receives the chunk means, may be
 * NULL.  Everything after the loads is float64; two-stage sums in a fixed
 * order through d_ws (cn_image_metrics_ws_bytes bytes; 0: arguments invalid),
 * no atomics: deterministic, and a view's numbers do not depend on V.
 * Returns -1 with cn_last_error() before any device call for H < 7, W < 7,
 * V < 1, chunk < 1, H * W > CN_MAX_SAMPLES, V > 65535 or a NULL d_img, d_gt,
 * d_out or d_ws. */
size_t cn_image_metrics_ws_bytes(int H, int W, int V, int chunk);
int cn_image_metrics(const float *d_img, const float *d_gt, int H, int W, int V, int chunk,
                     double *d_out, double *d_chunk_mse, void *d_ws, void *stream);

/* ---- torch.optim.AdamW step (src/trainer.py:116-120) over nseg tensors
 * (host arrays of device pointers), step = 1-based count of this update. */
int cn_adamw_step(int nseg, float *const *p, const float *const *g, float *const *m,
                  float *const *v, const int *n, const double *lr, double weight_decay,
                  double beta1, double beta2, double eps, int step, void *stream);
/* the same step, and every gradient element is set to 0 once read: the next
 * step's optimizer.zero_grad() (src/trainer.py:64) without a launch of its own */
int cn_adamw_step_zero_grad(int nseg, float *const *p, float *const *g, float *const *m,
                            float *const *v, const int *n, const double *lr, double weight_decay,
                            double beta1, double beta2, double eps, int step, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CODENERF_H */
