/*
 * dfepe.h — C ABI of libdfepe_hip.so: the MI355X (gfx950) weighted-8-point hot path of deepFEPE.
 *
 * The reference (eric-yyjau/pytorch-deepFEPE) is pure Python and has no FFI layer; the drop-in
 * boundary is therefore its Python call surface.  Each entry point below replaces
 * the arithmetic of the cited reference function; the Python mirror of that surface
 * (pytorch-deepfepe_amd/compat) binds these symbols with ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  Every pointer is a DEVICE pointer to
 *     contiguous fp32 (or int32 where stated) memory owned by the caller; nothing is allocated,
 *     freed or retained by the library; there is no global mutable state (re-entrant).
 *   - `stream` is a hipStream_t (NULL = default stream); work is enqueued asynchronously on it.
 *     The caller has made the owning device current (PyTorch does).
 *   - Return value: DFEPE_OK (0) or a negative DFEPE_ERR_* code; never throws.
 *   - Layouts follow the reference tensors: points [B,N,3] row-major, matrices [.,3,3] row-major
 *     flattened to 9, per-layer stacks [L,B,...].
 *   - Convention of F: x2^T F x1 = 0 (deepFEPE/models/DeepFNet.py:203-205).
 */
#ifndef DFEPE_H
#define DFEPE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFEPE_VERSION 154 /* 0.6.0 */

#define DFEPE_OK 0
#define DFEPE_ERR_INVALID_ARG (-1) /* null pointer, non-positive size, bad flag combination   */
#define DFEPE_ERR_HIP (-2)         /* a HIP runtime call failed (launch, attribute)            */
#define DFEPE_ERR_UNSUPPORTED (-3) /* valid request this build cannot serve (e.g. N too large) */

/* floats per pair in the `save` buffer handed from dfepe_w8pt_fwd to dfepe_w8pt_bwd.  The record is opaque and never outlives
   the process that wrote it: its inner layout may differ between builds of the library (csrc/w8pt16_body.h), and a backward that
   is handed a record of another layout returns NaN gradients instead of misreading it. */
#define DFEPE_SAVE_FLOATS 128

/* flags for dfepe_w8pt_fwd / dfepe_w8pt_bwd */
#define DFEPE_W8PT_RAW_MATCHES 1u /* `pts1` is matches_xy_ori [B,N,4] in pixels, `pts2` unused (may be NULL);
                                     the image-size normalisation of NormalizeAndExpand_HW is fused in   */
#define DFEPE_W8PT_LOGITS 2u      /* `weights` holds logits [B,N]; softmax over N (F.softmax(logits, dim=2),
                                     DeepFNet.py:443,512) is fused in and the weights are written to `weights_out`;
                                     the backward then returns the gradient w.r.t. the logits                */
/* variants of the textbook normalised 8-point solvers of dsac_tools (adjoint: dfepe_eight_point_bwd):       */
#define DFEPE_W8PT_SQRT2 4u       /* Hartley scale sqrt(2) (utils_F._normalize_XY, utils_F.py:23) instead of the
                                     literal 1.4142 of Fit.normalize                                         */
#define DFEPE_W8PT_NO_ROWNORM 8u  /* rows of the design matrix are not normalised to unit length
                                     (utils_F._E_from_XY / _F_from_XY, utils_F.py:122-130,239-247)           */
#define DFEPE_W8PT_FORCE_110 16u  /* singular values of the 3x3 forced to (1,1,0) instead of (s1,s2,0)
                                     (utils_F._E_from_XY, utils_F.py:148-149)                                */

#define DFEPE_W8PT_NO_HARTLEY 32u /* no Hartley normalisation, T1 = T2 = I (`normalize=False` of _E_from_XY /
                                     _F_from_XY, utils_F.py:116-119,233-236)                                 */

#define DFEPE_W8PT_ROW_PER_PAIR 64u /* scheduling only, same function, same `save` record: never spread a pair over the 16 rows of
                                       a cooperative workgroup (what the library does for 128 < N <= 2048: the forward fit of pixel
                                       matches up to 1280 pairs, of homogeneous points and the backward fit up to 3072; the rule
                                       is pytorch-deepfepe_amd/csrc/fit_plan.h);
                                       one 16-lane row per pair, correspondences re-read per phase.  A/B timing; pass the same
                                       bit to dfepe_w8pt_bwd or not, the record format does not depend on it.             */
#define DFEPE_W8PT_ALL_FLAGS 127u   /* any other bit in `flags` is DFEPE_ERR_INVALID_ARG                              */
#define DFEPE_W8PT16_MAX_N 128      /* largest N whose correspondences ONE row keeps in registers for the whole kernel; above it
                                       a cooperative workgroup per pair does (N <= 2048), or they are re-read per phase       */

int dfepe_version(void);
const char *dfepe_strerror(int code);
int dfepe_save_floats(void);

/* Self-test of the 16-lane row primitives the small-N solver kernels are built on (DPP row_newbcast / row_mirror /
 * row_half_mirror / quad_perm; pytorch-deepfepe_amd/csrc/rowgroup.h).  One wavefront: x, y [64] doubles in,
 * out [14][64] doubles: bcast<0>, bcast<5>, bcast<15>, row sum, sum of lanes 2..8, exchange partners 15-l, l^7, l^2, l^1,
 * fp32 row max, int32 row sum (of (int)(16 x)), y + bcast<3>(x) y, fp32 row sum, fp32 bcast<9> + int bcast<12> + lane id.
 * No counterpart in the reference; tests/test_rowgroup_gpu.py checks the hardware against these definitions. */
int dfepe_selftest_rowgroup(const double *x, const double *y, double *out, void *stream);

/*
 * Weighted normalised 8-point fit, forward.
 * Replaces: Fit.forward / Fit.weighted_svd / Fit.normalize (deepFEPE/models/DeepFNet.py:148-179,181-257,278-295),
 *           with DFEPE_W8PT_RAW_MATCHES also NormalizeAndExpand_HW (DeepFNet.py:93-120),
 *           and, when epi_res != NULL, utils_F.compute_epi_residual(pts1, pts2, out, clamp_at)
 *           (deepFEPE/dsac_tools/utils_F.py:400-413) as called in the recurrent loop (DeepFNet.py:479).
 *
 *   pts1, pts2 [B,N,3]  homogeneous points (pts*[:,:,2] is used exactly like the reference does), or
 *   pts1       [B,N,4]  pixel matches when DFEPE_W8PT_RAW_MATCHES (image_w/image_h = W,H of image_size)
 *   weights    [S,B,N]  S = n_weight_sets >= 1 weightings of the SAME B pairs (the reference's [B,1,N] is S = 1; S > 1
 *                       serves solver-only workloads that score several weightings per pair, e.g. all IRLS layers of a
 *                       fixed-logits step in one launch); every per-pair output then has a leading S dimension
 *   F_out      [B,9]    T2^T F' T1                          (reference `out`)
 *   residual   [B,N]    X f/|f|                             (reference `residual`)
 *   epi_res    [B,N]    or NULL
 *   save       [B,DFEPE_SAVE_FLOATS] or NULL (needed for backward); 16-byte aligned
 *   weights_out[B,N]    softmax(logits) when DFEPE_W8PT_LOGITS (may be NULL), ignored otherwise
 * Sign gauge: the reference inherits LAPACK's arbitrary sign of f; here f is oriented so that its
 * largest-magnitude component is positive (F_out and residual flip together, everything downstream is
 * sign-invariant).
 */
int dfepe_w8pt_fwd(const float *pts1, const float *pts2, const float *weights, int B, int N, int n_weight_sets,
                   unsigned flags, float image_w, float image_h, float clamp_at,
                   float *F_out, float *residual, float *epi_res, float *save, float *weights_out, void *stream);

/*
 * The same fit, handing the Hartley transforms of Fit.normalize from one launch to later ones.  Fit.normalize is unweighted: the
 * centroids and the scales 1.4142 / mean distance depend on the correspondences alone, so a step that fits the SAME matches at
 * several layers (every layer of pipeline.hot_path_fused; the recurrent model while it learns no offsets) computes them once.
 *   hartley      [B,DFEPE_HARTLEY_DOUBLES] doubles, 64-byte aligned: one record per pair of the B sets of correspondences (not per
 *                weight set); opaque, and like `save` it never outlives the step that wrote it
 *   hartley_mode DFEPE_HARTLEY_NONE   `hartley` is ignored (may be NULL): this call IS dfepe_w8pt_fwd
 *                DFEPE_HARTLEY_WRITE  the launch computes the transforms as always and also stores them (as fp64) in `hartley`
 *                DFEPE_HARTLEY_READ   the launch takes them from `hartley` instead of computing them
 * Every output is bit-identical in the three modes.
 * Contract: a reader must be given the same correspondences (pts1, pts2, B, N), the same image size and the same Hartley-affecting
 * flags (DFEPE_W8PT_RAW_MATCHES, DFEPE_W8PT_SQRT2, DFEPE_W8PT_NO_HARTLEY) as the writer, and the writer must come earlier on the
 * same stream.  Weights, DFEPE_W8PT_LOGITS and n_weight_sets may differ.  A reader that is handed a record no writer filled
 * returns NaN outputs instead of misreading it.
 * Where dfepe_w8pt_shares_hartley(N, flags) is 0 -- N > DFEPE_W8PT16_MAX_N, or DFEPE_W8PT_NO_HARTLEY -- both modes are ignored:
 * nothing is written, nothing is read, and the launch is that of dfepe_w8pt_fwd.  The answer depends on N and the flags only, never
 * on B, so a writer and its readers always agree.  DFEPE_HARTLEY_SHARE=0 in the environment (read once; A/B timing on one build)
 * makes this entry point ignore the record in both modes.
 * Errors (before any HIP call): a mode outside 0..2, or a non-zero mode with a NULL or misaligned `hartley`: DFEPE_ERR_INVALID_ARG
 * (checked first, whatever the shape and the switch above); then those of dfepe_w8pt_fwd.  B = 0 returns DFEPE_OK.
 * dfepe_version() stays 154 with this addition: the number is pinned by existing tests, and nothing that existed changes.
 */
#define DFEPE_HARTLEY_DOUBLES 8
#define DFEPE_HARTLEY_NONE 0
#define DFEPE_HARTLEY_WRITE 1
#define DFEPE_HARTLEY_READ 2
int dfepe_w8pt_fwd_shared(const float *pts1, const float *pts2, const float *weights, int B, int N, int n_weight_sets,
                          unsigned flags, float image_w, float image_h, float clamp_at,
                          float *F_out, float *residual, float *epi_res, float *save, float *weights_out,
                          double *hartley, int hartley_mode, void *stream);
int dfepe_w8pt_shares_hartley(int N, unsigned flags); /* 1 where a launch of this shape writes / reads the record */

/*
 * Backward of dfepe_w8pt_fwd w.r.t. the weights (analytic eigenvector / rank-2 / epipolar-residual
 * adjoints; replaces torch.autograd through the per-sample torch.svd calls, DeepFNet.py:232-256).
 *   g_F [B,9], g_residual [B,N], g_epi [B,N]: upstream gradients, each may be NULL (= zero)
 *   F_out: the forward output (needed when g_epi != NULL)
 *   g_weights_extra [B,N] or NULL: with DFEPE_W8PT_LOGITS, an upstream gradient on the `weights_out` tensor itself
 *     (the next estimator layer reads the weights, DeepFNet.py:487); added before the softmax adjoint
 *   with DFEPE_W8PT_LOGITS `weights` must be the forward's `weights_out` and g_weights receives d/d(logits)
 *   g_scale: device pointer to ONE float that multiplies the three upstream gradients (NULL = 1): the upstream gradient of a
 *     scalar loss whose d loss / d F was formed with unit upstream (dfepe_loss_tail), applied here because everything
 *     downstream of g_F, g_residual, g_epi is linear in them
 *   g_weights [B,N]: written (not accumulated)
 *   g_pts1, g_pts2 [B,N,3] or NULL: gradient w.r.t. the point coordinates (through the rows, the Hartley transforms and,
 *     when g_epi is given, the residual's direct dependence); with DFEPE_W8PT_RAW_MATCHES g_pts1 is [B,N,4] (gradient
 *     w.r.t. the pixel matches, 16-byte aligned) and g_pts2 is ignored.  NULL skips that part of the kernel.
 *   pending_loss_head: NULL, or the `workspace` of a dfepe_loss_tail(..., defer_head = 1) call enqueued earlier on the same
 *     stream: this launch then also finishes that call's loss head (packed / scalars), in spare wavefronts of its first
 *     workgroup where the kernel family allows it, as a kernel of its own behind it otherwise.  Pass it to exactly ONE
 *     backward launch of the step.
 */
int dfepe_w8pt_bwd(const float *pts1, const float *pts2, const float *weights, int B, int N, int n_weight_sets,
                   unsigned flags, float image_w, float image_h, float clamp_at,
                   const float *save, const float *F_out,
                   const float *g_F, const float *g_residual, const float *g_epi, const float *g_weights_extra,
                   const float *g_scale, float *g_weights, float *g_pts1, float *g_pts2, const void *pending_loss_head,
                   void *stream);

/*
 * Closing steps of the 8-point solvers for an EXPLICIT design matrix (dense-W form of the textbook solvers).
 * Replaces: the part of utils_F._E_from_XY / _F_from_XY after `XX = torch.mm(W, XX)` (deepFEPE/dsac_tools/utils_F.py:129-155,
 *           245-275) when W [N,N] is not diagonal: V[:, -1] of torch.svd(XX), the 3x3 step (S3 -> 0, or (1,1,0) with
 *           DFEPE_W8PT_FORCE_110), T2^T F T1.  A diagonal W is a per-correspondence weight: dfepe_w8pt_fwd serves it from the points.
 *   rows [B,N,9] design rows as the SVD sees them (already multiplied by W); T1, T2 [B,9] or both NULL (no de-normalisation);
 *   F_out [B,9].  flags: 0 or DFEPE_W8PT_FORCE_110.  Sign gauge as dfepe_w8pt_fwd.  Forward only.
 */
int dfepe_w8pt_rows_fwd(const float *rows, int B, int N, unsigned flags, const float *T1, const float *T2, float *F_out,
                        void *stream);

/*
 * F-loss and E-from-F over all layers.
 * Replaces: the per-layer body of get_all_loss_DeepF (deepFEPE/train_good_utils.py:325-358):
 *   pts*_eval = T* virt*^T ; losses = compute_epi_residual(pts1_eval, pts2_eval, F_layer, clamp_at) ;
 *   E_layer = K^T T2^T F_layer T1 K.
 *   F_layers [L,B,9]; T1,T2 [B,9] (t_stride = 9) or a single [9] shared by the batch (t_stride = 0);
 *   K [B,9]; virt1, virt2 [B,M,3]
 *   loss_sum [L,B]  = sum over the M virtual points of the clamped residual (caller divides by M / B)
 *   E_layers [L,B,9] or NULL
 */
int dfepe_floss_fwd(const float *F_layers, int L, int B, const float *T1, const float *T2, int t_stride,
                    const float *K, const float *virt1, const float *virt2, int M, float clamp_at,
                    float *loss_sum, float *E_layers, void *stream);

/*  g_loss_sum [L,B] or NULL, g_E [L,B,9] or NULL  ->  g_F_layers [L,B,9] (written).
 *  When g_loss_sum is NULL and g_loss_coef != 0 every entry of g_loss_sum is taken to be g_loss_coef * (*g_scale)
 *  (g_scale: device pointer to one float, NULL = 1): the adjoint of a plain mean over layers, pairs and points. */
int dfepe_floss_bwd(const float *F_layers, int L, int B, const float *T1, const float *T2, int t_stride,
                    const float *K, const float *virt1, const float *virt2, int M, float clamp_at,
                    const float *g_loss_sum, float g_loss_coef, const float *g_scale, const float *g_E,
                    float *g_F_layers, void *stream);

/*
 * Pose loss: decompose E^T into the two rotations / two translations, compare with the ground truth.
 * Replaces: the per-layer, per-sample loop of get_Rt_loss (deepFEPE/train_good_utils.py:96-239):
 *   utils_F._get_M2s (utils_F.py:478-498), utils_geo._R_to_q (utils_geo.py:58-86), _l2_error (:165-167),
 *   strict-'<' candidate selection (:160-168), rot12_to_angle_error (:150-155), vector_angle (:175-179).
 *   E_layers [L,B,9]; q_gt [B,4] (qs_cam); t_gt [B,3] (ts_cam, normalised inside); R_gt [B,9] = inv(delta)[:3,:3]
 *   q_l2, t_l2 [L,B]; R_deg, t_deg [L,B] (may be NULL); sel [L,B] int32 (bit0: R candidate, bit1: t candidate; may be NULL)
 */
int dfepe_pose_fwd(const float *E_layers, int L, int B, const float *q_gt, const float *t_gt, const float *R_gt,
                   float *q_l2, float *t_l2, float *R_deg, float *t_deg, int *sel, void *stream);

/*  g_q_l2, g_t_l2 [L,B] (either may be NULL) -> g_E [L,B,9] (written).
 *  When a gradient pointer is NULL and its coefficient is non-zero, the upstream gradient of that error is
 *  coef * (*g_scale) where the error is <= its clamp and 0 above it: the adjoint of
 *  clamp(stack(err), 0, clamp).mean() * balance  (deepFEPE/Train_model_pipeline.py:580-586) with coef = balance/(L*B). */
int dfepe_pose_bwd(const float *E_layers, int L, int B, const float *q_gt, const float *t_gt,
                   const float *g_q_l2, const float *g_t_l2, float coef_q, float clamp_q, float coef_t, float clamp_t,
                   const float *g_scale, float *g_E, void *stream);

/*
 * Loss head: reduce the per-pair sums to the scalars the training step uses.
 * Replaces: losses.mean() per layer / loss_F (train_good_utils.py:340-364) and the clamped qt mix
 * (Train_model_pipeline.py:580-586), plus the packed sums a data-parallel all-reduce needs.
 *   loss_sum [L,B] (sum over the M virtual points), q_l2, t_l2 [L,B] (may be NULL: no pose loss)
 *   packed   [L+4] doubles: sum_b loss_sum[l,b] (L), sum clamp(q), sum clamp(t), B, M
 *   scalars  [4+L] floats: loss = loss_F + loss_qt, loss_F, loss_qt, 0, then the L per-layer means   (local batch)
 */
int dfepe_loss_head(const float *loss_sum, const float *q_l2, const float *t_l2, int L, int B, int M,
                    float clamp_q, float clamp_t, float balance_q, float balance_t,
                    double *packed, float *scalars, void *stream);

/*
 * The whole loss tail of the hot-path step in ONE launch (one 16-lane row per pair): dfepe_floss_fwd + E-from-F +
 * dfepe_pose_fwd + dfepe_loss_head, and -- when g_F_layers != NULL -- dfepe_pose_bwd + dfepe_floss_bwd for
 *     loss = balance_F * mean_{l,b,m}(F-loss) + balance_q * mean_{l,b}(clamp(q_l2, 0, clamp_q)) + balance_t * mean_{l,b}(clamp(t_l2, 0, clamp_t))
 * with unit upstream gradient (every coefficient of such a loss is a constant: the adjoint of a term is formed where its
 * forward value is).  Replaces: get_all_loss_DeepF's per-layer body (deepFEPE/train_good_utils.py:325-358), get_Rt_loss's
 * loop (:96-239) and the loss mixing of Train_model_pipeline.py:580-587 (which uses balance_F = 0 when if_qt_loss).
 *   arguments as in dfepe_floss_fwd / dfepe_pose_fwd / dfepe_loss_head; M <= 128 (else DFEPE_ERR_UNSUPPORTED: use those)
 *   q_gt == NULL: no pose part (then t_gt, q_l2, t_l2, R_deg, t_deg, sel are ignored)
 *   grad_pairs: number of pairs the means run over in the gradient coefficients (B, or the global batch under data parallelism)
 *   g_F_layers [L,B,9] or NULL; feed it to dfepe_w8pt_bwd with g_scale = the upstream gradient of the loss
 *   packed [L+4] doubles, scalars [4+L] floats: as dfepe_loss_head, scalars[0] = balance_F * loss_F + loss_qt
 *   workspace: dfepe_loss_tail_workspace_bytes(B) bytes, 16-byte aligned, contents irrelevant (per-workgroup partial sums;
 *     a one-workgroup kernel enqueued right behind adds them in a fixed order: no floating-point atomics, deterministic)
 *   defer_head: 0 = packed / scalars are complete when this call's work is (two launches).  1 = only the per-pair outputs
 *     and g_F_layers are; the batch sums are left pending in `workspace` and finished by the dfepe_w8pt_bwd launch that is
 *     handed `workspace` as its pending_loss_head (same stream, before packed / scalars are read).  For a training step
 *     whose backward follows at once (a captured graph): the backward does not need the scalars, and the head's launch
 *     (~7 us) leaves the step's critical path.
 */
size_t dfepe_loss_tail_workspace_bytes(int B);
int dfepe_loss_tail(const float *F_layers, int L, int B, const float *T1, const float *T2, int t_stride, const float *K,
                    const float *virt1, const float *virt2, int M, float clamp_at,
                    const float *q_gt, const float *t_gt, const float *R_gt, float clamp_q, float clamp_t,
                    float balance_F, float balance_q, float balance_t, double grad_pairs,
                    float *loss_sum, float *E_layers, float *q_l2, float *t_l2, float *R_deg, float *t_deg, int *sel,
                    float *g_F_layers, double *packed, float *scalars, void *workspace, int defer_head, void *stream);
/* The pending loss head of a dfepe_loss_tail(..., defer_head = 1) call as a launch of its own, on any stream ordered after that
 * call (instead of riding in a dfepe_w8pt_bwd launch): lets the head and the data-parallel all-reduce of `packed` that follows it
 * run on a side stream while the backward fits run on the main one.  `workspace`: the one given to dfepe_loss_tail. */
int dfepe_loss_head_pending(const void *workspace, void *stream);

/*
 * The loss tail behind the reference's OWN call sequence (get_all_loss_DeepF, then get_Rt_loss, then the caller's clamp /
 * balance mixing in torch, Train_model_pipeline.py:508-586): the coefficients of the loss are not known when the forward
 * runs, so this variant of dfepe_loss_tail leaves, next to the same per-pair outputs, the three JACOBIANS of every
 * (layer, pair):  J [L,B,27] = d loss_sum / dF (9) | d q_l2 / dF (9) | d t_l2 / dF (9)   (unclamped, unit upstream),
 * and dfepe_loss_tail_bwd turns whatever upstream gradients autograd delivers into d loss / dF in one launch:
 *   g_F[l,b] = g_loss_sum[l,b] J_F + g_q_l2[l,b] J_q + g_t_l2[l,b] J_t        (each upstream pointer may be NULL = zero;
 *   gradients that arrive on the batch statistics of dfepe_loss_stats enter through g_mean_* / g_all_*, see there)
 * Replaces: torch.autograd through get_all_loss_DeepF's per-layer body (deepFEPE/train_good_utils.py:325-358) and
 *           get_Rt_loss's per-sample loop (:96-239).  No batch sums here (the caller's torch means take them).
 *   arguments as in dfepe_loss_tail, M <= 112 (else DFEPE_ERR_UNSUPPORTED); q_gt == NULL: no pose part (J_q = J_t = 0); want_floss_jac == 0: J_F = 0 and the F-loss
 *   adjoint work is skipped (an objective without the F-loss, the reference's if_qt_loss)
 */
int dfepe_loss_tail_jac(const float *F_layers, int L, int B, const float *T1, const float *T2, int t_stride, const float *K,
                        const float *virt1, const float *virt2, int M, float clamp_at,
                        const float *q_gt, const float *t_gt, const float *R_gt, int want_floss_jac,
                        float *loss_sum, float *E_layers, float *q_l2, float *t_l2, float *R_deg, float *t_deg, int *sel,
                        float *J, void *stream);
int dfepe_loss_tail_bwd(const float *J, int L, int B, const float *g_loss_sum, const float *g_q_l2, const float *g_t_l2,
                        const float *g_mean_loss, const float *g_all_loss, const float *g_mean_q, const float *g_all_q,
                        const float *g_mean_t, const float *g_all_t, float stat_loss_scale, float *g_F_layers, void *stream);

/*
 * Batch statistics of the per-pair loss terms in one launch.
 * Replaces: the per-layer `.mean()` calls and python sums of get_all_loss_DeepF (deepFEPE/train_good_utils.py:343-364: losses.mean()
 *           per layer, loss_F = sum / len, loss_min_layers / loss_min_batch :375-376, loss_epi_res :429-438) and of get_Rt_loss
 *           (:272-283: x.mean() per layer, mean_list) -- a dozen small reductions in the reference's style, one launch here.
 *   up to four sets k of rows x_k [rows_k, C] (rows_k = 0: absent; rows_k <= 64), C = pairs
 *   out: for every present set in order, rows_k floats = scale_k * mean over C of each row, then 1 float = the mean of those
 *   row_min0 [rows0] or NULL: scale0 * min over C of each row of set 0; col_min0 [C] or NULL: scale0 * min over the rows of set 0
 * dfepe_loss_tail_bwd's g_mean_* [L] / g_all_* [1] take the gradients of such row means / of their mean for the sets loss_sum
 * (scale = stat_loss_scale), q_l2, t_l2 directly: no expansion of a mean's gradient to [L,B] in between.
 */
int dfepe_loss_stats(const float *x0, int rows0, float scale0, const float *x1, int rows1, float scale1,
                     const float *x2, int rows2, float scale2, const float *x3, int rows3, float scale3, int C,
                     float *out, float *row_min0, float *col_min0, void *stream);

/*
 * Cheirality-checked pose from E.
 * Replaces: utils_F._E_to_M_train (deepFEPE/dsac_tools/utils_F.py:679-763): the four candidates of _get_M2s in
 * the order (R1,t),(R1,-t),(R2,t),(R2,-t), linear triangulation of every correspondence (the reference calls
 * cv2.triangulatePoints), count of points with 0 < Z < depth_thres in both cameras, first arg-max wins.
 *   E [B,9]; K [B,9]; matches [B,N,4] pixels
 *   pre [B,9] or NULL: when given, the matrix decomposed is pre^T E pre -- pass E = F (the fit's output) and pre = T K to fuse
 *     E-from-F (E = K^T T^T F T K, train_good_utils.py:356-358) into this launch
 *   Rt_cam [B,12]  inverse (camera motion) of the winner, zeros when no candidate has a valid point
 *   winner [B] int32 (-1 when none); counts [B,4] int32
 * Arithmetic: the DLT null vector of every (correspondence, rotation) in packed fp32; a correspondence whose depth tests lie
 * within that vector's a-posteriori error bound of a threshold is decided by the fp64 route instead (fp64 normal matrix + one
 * Rayleigh-quotient iteration), so the counts are those of an fp64 DLT.
 */
int dfepe_cheirality(const float *E, const float *pre, const float *K, const float *matches, int B, int N, float depth_thres,
                     float *Rt_cam, int *winner, int *counts, void *stream);
/* The same with flags and an optional workspace.
 * DFEPE_CHEIR_FP64_ONLY: every correspondence takes the fp64 route (no packed-fp32 decisions): the build the adaptive default is
 *   tested against for EXACT equality of the counts (tests/test_fullsize_gpu.py), and its upper bound in time.
 * workspace: NULL, or dfepe_cheirality_workspace_bytes(B) bytes of device memory (8-byte aligned, overwritten).  With it the
 *   per-pair constants of the correspondence loop (the decomposition of E, the two candidate projection matrices K [R|t]) are
 *   formed by a preparation launch with one LANE per pair and fetched by the main kernel through scalar loads, instead of being
 *   re-derived by every wavefront (a closed-form fp64 SVD issued for 64 lanes: ~12 % of the launch at one wavefront per pair).
 *   Same outputs bit for bit. */
#define DFEPE_CHEIR_FP64_ONLY 1u
size_t dfepe_cheirality_workspace_bytes(int B);
int dfepe_cheirality_ex(const float *E, const float *pre, const float *K, const float *matches, int B, int N, float depth_thres,
                        unsigned flags, void *workspace, float *Rt_cam, int *winner, int *counts, void *stream);

/*
 * Fit + E-from-F + cheirality-checked pose in one call (BASELINE config 5: one weighted 8-point fit, then the pose of its F).
 * Replaces: Fit.forward -> E = K^T T^T F T K (train_good_utils.py:356-358) -> utils_F._E_to_M_train (utils_F.py:679-763).
 * Same outputs as dfepe_w8pt_fwd (DFEPE_W8PT_RAW_MATCHES required; DFEPE_W8PT_LOGITS optional; no `save`: forward only) followed
 * by dfepe_cheirality(F_out, pre, ...), bit for bit; for 128 < N <= 2048 up to 1280 pairs (where the forward fit of pixel matches
 * takes the cooperative workgroup: fit_pose_fused, pytorch-deepfepe_amd/csrc/fit_plan.h) it is ONE launch (that workgroup goes on to
 * decompose pre^T F pre and to triangulate its pair), otherwise the two launches.
 * workspace: NULL or dfepe_cheirality_workspace_bytes(B) bytes, handed to dfepe_cheirality_ex when the two launches run.
 */
int dfepe_w8pt_pose_fwd(const float *matches, const float *weights, int B, int N, unsigned flags, float image_w, float image_h,
                        float clamp_at, const float *K, const float *pre, float depth_thres, float *F_out, float *residual,
                        float *epi_res, float *weights_out, float *Rt_cam, int *winner, int *counts, void *workspace, void *stream);

/*
 * Reductions of the validation summary on the device.
 * Replaces: the numpy post-processing of write_metrics_summary (deepFEPE/train_good_utils.py:758-856) over the per-pair
 * results of val_rt (:553-646): epipolar-distance inlier ratios at 0.1 / 1.0 px, F1 of "est < th" against "gt < th",
 * medians and maxima of the pose errors, np.histogram counts of the errors over the thresholds
 * 0, 0.01, 0.03, 0.05, 0.1, 0.3, 0.5, 1, 2, 5, 10, 90, 180 degrees.
 *   epi_est, epi_gt [n_epi] epipolar distances of every correspondence under the estimated / ground-truth F (epi_gt may be NULL)
 *   err_q, err_t [B] rotation / translation errors in degrees
 *   out: dfepe_metrics_summary_bytes() bytes, 8-byte aligned, overwritten:
 *     uint64 counts[8]  = #est<0.1, #est<1, (TP, FP, FN) at 0.1, (TP, FP, FN) at 1.0
 *     uint64 hist[2][12] bin counts for err_q, err_t (bins [th_k, th_k+1), the last closed; values outside [0,180] dropped)
 *     float  max[2], float mids[2][2] = the two middle order statistics of err_q, err_t (median = their mean)
 *   comparisons: est, gt against 0.1f and 1.0f in float32; the histogram in float64 against the float64 thresholds, as
 *     np.histogram does (a float32 error next to a rounded threshold lands where numpy puts it)
 *   max: the largest entry that is > 0, NaN if any entry is NaN, +0.0 otherwise (-0.0 and negative entries never win: np.amax of
 *     a vector with one entry >= 0); mids: NaN if any entry is NaN
 *   median: the caller forms 0.5 * (mids[0] + mids[1]) in float64 and does NOT round it back to float32 -- np.median of the errors
 *     widened to float64; np.median of the float32 vector would round the mean
 *   B = 0 or n_epi = 0: nothing is launched for that half, its part of the record stays zero
 * Raw counts, not ratios: the host derives the ratios after ONE device-to-host copy per validation epoch.
 */
size_t dfepe_metrics_summary_bytes(void);
int dfepe_metrics_summary(const float *epi_est, const float *epi_gt, size_t n_epi, const float *err_q, const float *err_t,
                          int B, void *out, void *stream);

/*
 * Epipolar metrics of dsac_tools.utils_F (utils_F.py:291-361) on homogeneous-or-not 2-D points.
 *   kind: 0 = _sym_epi_dist (squared; `eps` is added to the two squared line norms: 1e-10 in the reference's batched branch,
 *         0 in its 2-D branch), 1 = _sampson_dist, 2 = _epi_distance (writes 3 planes: mean, d1, d2);
 *         | DFEPE_EPI_HOMOGENEOUS: X, Y are [B,N,3] homogeneous points used as they are (if_homo=True), else [B,N,2]
 *   F [B,9]; out [B,N] (kind 0,1) or [3,B,N] (kind 2); clamp_at < 0 means no clamp (clamp_at=None; kind 0 only)
 *   a point with F x = 0 (or F^T y = 0) gives what the float64 formula gives, NaN (0 * inf, 0 / 0) included; the clamp keeps a NaN,
 *   as torch.clamp does
 */
#define DFEPE_EPI_HOMOGENEOUS 8
int dfepe_epi_metrics(int kind, const float *F, const float *X, const float *Y, int B, int N, float clamp_at,
                      float eps, float *out, void *stream);

/*
 * Stand-alone symmetric epipolar residual (the same arithmetic dfepe_w8pt_fwd fuses in its epilogue).
 * Replaces: utils_F.compute_epi_residual(pts1, pts2, F, clamp_at) (deepFEPE/dsac_tools/utils_F.py:400-413).
 *   pts1, pts2 [B,N,3]; F [B,9]; out [B,N].   bwd: g_out [B,N] -> g_F [B,9] (gradient w.r.t. F only).
 */
int dfepe_epi_residual_fwd(const float *pts1, const float *pts2, const float *F, int B, int N, float clamp_at,
                           float *out, void *stream);
int dfepe_epi_residual_bwd(const float *pts1, const float *pts2, const float *F, int B, int N, float clamp_at,
                           const float *g_out, float *g_F, void *stream);

/*
 * Small pose-geometry helpers, batched over n items (one lane each).
 *   kind 0  rotation -> quaternion          in0 = R [n,9]              out [n,4]   (utils_geo._R_to_q, utils_geo.py:58-86)
 *   kind 1  rotation angle in degrees       in0 = R0 [n,9], in1 = R1   out [n]     (utils_geo.rot12_to_angle_error, :150-155)
 *   kind 2  vector angle in degrees         in0 = v1 [n,3], in1 = v2   out [n]     (utils_geo.vector_angle, :175-179)
 *   kind 3  singular values forced to 1,1,0 in0 = E [n,9]              out [n,9]   (utils_F._F_to_E projection, utils_F.py:457-461;
 *                                                                                   Train_model_pipeline.py:954-964)
 *   kind 4  four-fold decomposition         in0 = E [n,9]              out [n,21] = R1[9] R2[9] t[3]
 *                                                                                  (utils_F._get_M2s, utils_F.py:478-498)
 *   kind 5  congruence A^T F A              in0 = F [n,9], in1 = A [n,9] out [n,9]  (E = K^T T2^T F T1 K with A = T K when
 *                                                                                   T1 = T2: train_good_utils.py:356-358,366-369;
 *                                                                                   utils_F._F_to_E's K^T F K, utils_F.py:456)
 *   kind 6  camera rotation of a scene motion  in0 = delta [n,16]       out [n,9] = inv(delta)[:3,:3]
 *                                                                                  (get_Rt_loss, train_good_utils.py:134,170)
 * Kind 2 is the reference's formula acos(clip(v1.v2 / ((|v1| + 1e-10)(|v2| + 1e-10) + 1e-10))) as it stands: at |v| ~ 1 the three
 * 1e-10 terms leave the cosine of parallel vectors at 1 - 3e-10, so equal vectors report about 1.4e-3 degrees (opposite ones
 * 180 - 1.4e-3) and every near-parallel direction error carries that floor; 0 and 180 come out exactly only where the terms are
 * absorbed (|v| >~ 1e6).  A zero vector reports 90.
 * Every kind computes in float64 from the float32 inputs and rounds once.  A NaN in an item's inputs makes that item's outputs NaN
 * and touches no other item (kinds 3 and 4: any NaN or infinity in E makes all of the item's outputs NaN).  Kinds 3 and 4 return
 * orthonormal factors for every finite E, a rank-1 or zero matrix included, where the projection itself is not defined.
 */
int dfepe_geo_misc(int kind, const float *in0, const float *in1, int n, float *out, void *stream);

/*
 * Inputs of the recurrent model from the pixel matches.
 * Replaces: DeepFNet.get_input (deepFEPE/models/DeepFNet.py:362-391) with NormalizeAndExpand_HW (:93-120): the image-size
 *           normalisation T_HW (x, y, 1) of both point sets and the estimator's input channels ((x+1)/2, (y+1)/2 of both images,
 *           then the Q quality channels) -- about fifteen elementwise / bmm launches in the reference, one here.
 *   matches [B,N,4] pixels (16-byte aligned); quality [B,N,Q] or NULL (Q = 0)
 *   weight_in or NULL: element (copy k, channel c < 4+Q, pair b, point i) goes to
 *     weight_in[k * copy_stride + c * channel_stride + b * batch_stride + i], k < n_copies.  The reference's [B,4+Q,N] tensor is
 *     channel_stride = N, batch_stride = (4+Q) N; channel-major storage [C,B,N] (channel_stride = B N, batch_stride = N) lets the
 *     fit kernels write the recurrent channels (weights, epipolar residual, residual) of the next estimator input as plain
 *     [B,N] blocks, and n_copies fills the point channels of every layer's input buffer in this one launch (no torch.cat per
 *     layer, DeepFNet.py:484-489)
 *   pts1, pts2 [B,N,3] or NULL: homogeneous normalised points (the arithmetic of dfepe_w8pt_fwd's DFEPE_W8PT_RAW_MATCHES prologue)
 */
int dfepe_deepf_input(const float *matches, const float *quality, int B, int N, int Q, float image_w, float image_h,
                      float *weight_in, size_t channel_stride, size_t batch_stride, int n_copies, size_t copy_stride,
                      float *pts1, float *pts2, void *stream);

/*
 * Per-pair dot products of two per-layer stacks: out[l,b] = sum_n a[l,b,n] * b[l,b,n].
 * Replaces: the `epi_res * weights` products under loss_epi_res (deepFEPE/train_good_utils.py:429-438), whose means
 *           dfepe_loss_stats then takes as one more row set.
 *   a, b: n_layers blocks of [B,N] floats, block l at a + l * a_layer_stride (resp. b + l * b_layer_stride): the layers may
 *   live in separate per-layer buffers a fixed distance apart (the channel-major estimator inputs of dfepe_deepf_input);
 *   out [n_layers,B]
 */
int dfepe_row_dot(const float *a, size_t a_layer_stride, const float *b, size_t b_layer_stride, int n_layers, int B, int N,
                  float *out, void *stream);

/*
 * InstanceNorm1d(affine) + LeakyReLU on rows of N contiguous floats ("next" row f-1: the part of the weight estimator
 * between its 1x1 convolutions, deepFEPE/models/ErrorEstimators.py:47-64; the convolutions themselves are GEMMs).
 *   Y, A, gA, gY: [(c*R + r)*N + n]  (channel-major: c < C channels, r < R rows per channel, N points), 16-byte aligned;
 *   gamma, beta [C]; stats [C*R*2] = (mean, 1/sqrt(var+eps)) per row, written by fwd and read by bwd;
 *   row_ggamma, row_gbeta [C*R]: per-row contributions to d/d(gamma[c]), d/d(beta[c]) (sum over r is left to the caller).
 *   N must be a multiple of 4 and <= 512 (DFEPE_ERR_UNSUPPORTED otherwise).
 */
int dfepe_inorm_lrelu_fwd(const float *Y, const float *gamma, const float *beta, int C, int R, int N, float eps, float slope,
                          float *A, float *stats, void *stream);
int dfepe_inorm_lrelu_bwd(const float *Y, const float *gA, const float *gamma, const float *beta, const float *stats,
                          int C, int R, int N, float slope, float *gY, float *row_ggamma, float *row_gbeta, void *stream);

/*
 * The weight estimator on the matrix cores, N = dfepe_est_points() = 100 points per pair.
 * Replaces: ErrorEstimator.forward, the Conv1d(k=1) -> InstanceNorm1d(affine) -> LeakyReLU stack and its autograd backward
 *           (deepFEPE/models/ErrorEstimators.py:47-64, called at deepFEPE/models/DeepFNet.py:441,510).
 * Every fp32 operand travels as 16-bit PLANES, exact remainders of each other.  Forward products (round 5): TWO fp16 planes per
 * operand (22 mantissa bits), three MFMAs (a0 b0 + a0 b1 + a1 b0, fp32 accumulate): fp32-class accuracy at half the matrix work of
 * the six bf16 products of rounds 3-4; a layer's weights are split scaled by the power of two that brings max |W| into [8, 16)
 * (their low plane would otherwise sit in fp16's subnormal range), the accumulators are scaled back before the statistics.
 * Backward products: two bf16 planes each (three MFMAs, ~2^-16; gradients keep bf16's range without any loss scaling), so a
 * forward layer that will be differentiated also leaves its activation as two bf16 planes.  Domain: |activation| <= 65504 (fp16;
 * InstanceNorm bounds it by |gamma| sqrt(N - 1) + |beta|) -- beyond it the logits are NaN, not silently wrong.
 * Plane buffers are 16-bit, POINT-major and K-blocked: element (row, ch) of a plane with `rows` rows
 * lives at ((ch / 32) * rows + row) * 32 + ch % 32; `*_plane` arguments are the element strides between planes; ncols = pairs * 100.
 *   dfepe_est_split      fp32 [rows][C_src] (ld = src_ld) -> n_planes bf16 planes with C (% 32 == 0) channels, the tail zero
 *   dfepe_est_absmax     *word = max(*word, bit pattern of max |src[i]|) -- the caller zeroes the word first; the scale of
 *                        dfepe_est_split_f16 / dfepe_est_layer_fwd / dfepe_est_gemm_nt_f16 is derived from it on the device
 *   dfepe_est_wprep      (version 152) the weights of n_layers <= 8 layers (host arrays of device pointers W[l] [Co[l]][Ci[l]]) in two
 *                        launches: words[l] = bit pattern of max |W[l]| (partial maxima in `workspace`, dfepe_est_wprep_workspace_bytes
 *                        bytes, contents irrelevant: no atomics, no zeroing), then
 *                        planes_f16[l] = two fp16 planes [Co][K = Ci rounded up to 32] of W[l] scaled as in dfepe_est_split_f16 and,
 *                        where planes_wt (and planes_wt[l]) is not null, two bf16 planes of W[l]^T [K][Co] (Co % 32 == 0) -- what
 *                        dfepe_est_gemm_nt / dfepe_est_dgrad_in_bwd multiply dY by.  At the reference's batch sizes (4-32 pairs) a
 *                        call's bookkeeping launches (per layer: maximum, split, transposed split, reductions, fills) cost more
 *                        than its GEMMs; this and dfepe_est_colsum take one estimator call from ~75 launches to ~30
 *   dfepe_est_colsum     dst[s][c] = sum_r src[s][r * cols[s] + c], r < rows[s], for n_seg <= 40 segments in ONE launch, additions in a
 *                        fixed order (rows[s] = 0: zeros, src[s] may be null): all reductions of one backward -- per-pair d gamma /
 *                        d beta partials, split-K partials of the weight gradients -- and the zero gradients of the cancelled biases
 *   dfepe_est_split_f16  the same into two fp16 planes, the values multiplied by the scale of `absmax` (null: unscaled)
 *   dfepe_est_layer_fwd  planes_out[2][...M] (fp16) = split(leaky_relu(instance_norm(W X) * gamma + beta)), planes_bwd[2][...M]
 *                        (bf16; null when no gradient is wanted) the same activation for the backward; rstd [pairs][M];
 *                        W planes [2] of [M][K] split with `absmax` (or null), X planes [2] of [ncols][K], both fp16; the
 *                        convolution bias cancels in the normalisation
 *   dfepe_est_gemm_nt    out[col][m] (fp32, ld = ldc) = sum_k A[m][k] B[col][k] on n_planes (2 or 3) bf16 planes: the data
 *                        gradient dA = W^T dY
 *   dfepe_est_gemm_nt_f16  the forward's plain product on two fp16 planes each, A split with `absmax` (or null)
 *   dfepe_est_gemm_tn    part[slices][Cout][Cin] = split-K partial sums of dW = dY^T X (two planes each; the caller adds the slices)
 *   dfepe_est_in_bwd     dY planes [2] = adjoint of InstanceNorm + LeakyReLU given dA [ncols][C] fp32 (or its rank-one head form
 *                        dlogit[col] * w_head[c]), the layer's output planes [2] (bf16), rstd, gamma, beta; per-pair d gamma / d beta
 *   dfepe_est_dgrad_in_bwd  (round 5) the data gradient dA = dY_next W_next (WT = W_next^T planes [2] of [M][K], dY_next planes [2] of
 *                        [ncols][K], bf16) and dfepe_est_in_bwd of the layer below in ONE launch: dA stays in the accumulators (two
 *                        whole pairs x 128 channels per workgroup), the layer's output planes are read twice (statistics, then dY),
 *                        dY planes [2], per-pair d gamma / d beta out.  dA never reaches memory: 8 of the 20 bytes per element the
 *                        two launches moved.  N = dfepe_est_points() only
 *   dfepe_est_norm_fwd   any N points per pair (the reference's SIFT configurations: up to 2000): planes_out [2] (fp16), planes_bwd
 *                        [2] (bf16, or null) and rstd from the plain product Y fp32 [n_pairs * N][ldy] of dfepe_est_gemm_nt_f16 --
 *                        InstanceNorm (biased variance, two-pass),
 *                        affine, LeakyReLU, split; dfepe_est_layer_fwd is this fused into the product for N = dfepe_est_points().
 *                        splits = 1: one launch, a workgroup per (pair, 64 channels); splits in 2..64 (a dozen pairs do not fill the
 *                        chip): each pair's rows over `splits` workgroups in two launches (partial mean / squared deviations, merged
 *                        pairwise; then the normalisation), part = workspace of n_pairs * splits * 2 * C floats
 *   dfepe_est_in_bwd_n   dfepe_est_in_bwd for any N (ncols = n_pairs * N)
 *   dfepe_est_dgamma_zero  the two adjoints above recover x^ as (z - beta) / gamma and take it as 0 where gamma is exactly 0 (their
 *                        d beta and dY are right there, d gamma is not): this launch, run after them, overwrites dgamma_part[pair][ch]
 *                        of every channel with |gamma| < 1e-30 from a recomputation of the layer's product (input planes [2], bf16, of
 *                        [ncols][K-blocked], fp32 weights W [C][ldw], Ci input channels); channels with gamma != 0 cost an idle
 *                        workgroup each.  N <= 4096.  The upstream gradient comes from dA, from the head's rank-one form, or -- behind
 *                        dfepe_est_dgrad_in_bwd, which never writes dA -- is recomputed for the channel from dY_next planes [2] of
 *                        [ncols][C_next] and the next layer's fp32 weights W_next [C_next][ldw_next].  dfepe_est_dgamma_zero_multi: the
 *                        same for n_layers <= 8 layers in ONE launch (host arrays indexed by layer; ldw = Ci, ldw_next = C)
 *   dfepe_est_forward / dfepe_est_backward  (version 153) ONE call per estimator pass: the whole stack of n_hidden <= 8 layers and its
 *                        one-channel head through the entry points above, in the order the host code used to issue them (bit-identical
 *                        results).  x [B][C0][N], W[l] [Co[l]][Ci[l]] (Ci[l] = Co[l-1], Ci[0] = C0; Co % 32 == 0), gamma / beta [l]
 *                        [Co[l]], w_head [Co of the last layer], b_head [1] or null: fp32, contiguous, host arrays of device pointers.
 *                        The caller brings the memory: `saved` (dfepe_est_saved_bytes; null for a forward no backward will follow; what
 *                        the backward reads: every layer's bf16 planes, reciprocal deviations, transposed weight planes; need_gx does not
 *                        change its layout -- a backward may ask for gx or not), a transient workspace per pass (dfepe_est_*_workspace_bytes;
 *                        16-byte aligned, contents irrelevant) and the outputs: logits [B * N]; g_W[l] [Co][Ci], g_bias[l] [Co] (exact
 *                        zeros: the convolution bias cancels in the normalisation), g_gamma[l], g_beta[l] [Co], g_w_head, g_b_head
 *                        (or null), gx [B][C0][N] (or null).  N = dfepe_est_points() takes the fused epilogues, any other N >= 2 the
 *                        plain products.  Why: at the reference's batch sizes the HOST was the limiter of the eager training step
 *                        (~30 launches and ~40 allocations per pass from Python)
 *   dfepe_est_head_fwd   logits[col] = sum_c w[c] a[col][c] + bias[0]   (the last Conv1d(C -> 1)); a: the forward's planes [2] (fp16)
 *   dfepe_est_head_dw    part[blocks][C] = partial sums of d w = sum_col dlogit[col] a[col][c]; a: the backward's planes [2] (bf16);
 *                        bias_part [blocks] (or null; version 154) = partial sums of dlogit: the head bias gradient's, in the same launch
 * Version 154 (round 6) -- the reference's own shapes (N = 1000-2000 points, 4-12 pairs per batch, deepFEPE/configs/kitti_corr_baseline.yaml:12-13)
 * and an estimator that one model forward calls several times (DeepFNet.update_weights, deepFEPE/models/DeepFNet.py:510):
 *   dfepe_est_gemm_nt_f16_splitk / dfepe_est_gemm_nt_splitk   the plain products with their K steps shared by `splits` workgroups per tile:
 *                        partial products out[z][col][m], z < splits <= K / 32, split_stride (>= ncols * ldc) floats apart.  With a few
 *                        pairs per batch a K-heavy layer is a dozen 128 x 208 tiles: a chain of 16-32 K steps on 5 % of the chip
 *   dfepe_est_norm_fwd_r / dfepe_est_in_bwd_r   dfepe_est_norm_fwd / dfepe_est_in_bwd_n for N <= 2048 with the pair's block RESIDENT IN
 *                        REGISTERS: one launch, one read of the product, given as `splits` partials (added in slice order); a workgroup =
 *                        one pair x 32 channels
 *   dfepe_est_gemm_nt_gx the data gradient of the FIRST layer stored as the estimator's input gradient: element (pair, ch, n) at
 *                        pair * gx_stride_pair + ch * gx_stride_ch + n (was: a transposing launch behind the plain product).  x and gx of
 *                        dfepe_est_forward / dfepe_est_backward take the same two strides: dense [B][C0][N] (C0 N, N) or a view of the
 *                        channel-major [C0][B][N] buffers compat.DeepFNet keeps its estimator inputs in (N, B N) -- no copies
 *   dfepe_est_gemm_tn_multi   dfepe_est_gemm_tn for n_layers <= 8 layers over the same columns in ONE launch (host arrays indexed by layer)
 *   dfepe_est_prep_bytes / dfepe_est_prepare   the weights' planes of one estimator (power-of-two scales, scaled fp16 planes, transposed
 *                        bf16 planes) into a caller-owned buffer `prep`, two launches; dfepe_est_forward / dfepe_est_backward given
 *                        `prep` read them instead of making their own per call.  The weights must not change between dfepe_est_prepare
 *                        and the last backward handed `prep` (one optimizer step apart at the earliest)
 *   dfepe_est_forward / dfepe_est_backward   take `prep` (or null); per layer they run the fused epilogue (N = dfepe_est_points(), enough
 *                        tiles) or plain product -> dfepe_est_norm_fwd_r / dfepe_est_in_bwd_r (any other N <= 2048, and K-heavy layers
 *                        on few tiles, split over K) -- or the strided kernels beyond N = 2048; over few columns the weight gradients of
 *                        all layers are one dfepe_est_gemm_tn_multi launch at the end of the backward
 */
int dfepe_est_points(void);
int dfepe_est_split(const float *src, long rows, int C_src, int src_ld, int C, int n_planes, void *planes, size_t plane_stride,
                    void *stream);
int dfepe_est_absmax(const float *src, long n, unsigned *word, void *stream);
size_t dfepe_est_wprep_workspace_bytes(int n_layers);
int dfepe_est_wprep(int n_layers, const float *const *W, const int *Co, const int *Ci, void *const *planes_f16,
                    void *const *planes_wt, unsigned *words, void *workspace, void *stream);
int dfepe_est_colsum(int n_seg, const float *const *src, const int *rows, const int *cols, float *const *dst, void *stream);
int dfepe_est_split_f16(const float *src, long rows, int C_src, int src_ld, int C, const unsigned *absmax, void *planes,
                        size_t plane_stride, void *stream);
int dfepe_est_layer_fwd(const void *W, size_t w_plane, const void *X, size_t x_plane, int M, int ncols, int K,
                        const unsigned *absmax, const float *gamma, const float *beta, float eps, float slope, void *planes_out,
                        size_t out_plane, void *planes_bwd, size_t bwd_plane, float *rstd, void *stream);
int dfepe_est_gemm_nt_f16(const void *A, size_t a_plane, const void *B, size_t b_plane, int M, int ncols, int K,
                          const unsigned *absmax, float *out, int ldc, void *stream);
int dfepe_est_gemm_nt(const void *A, size_t a_plane, const void *B, size_t b_plane, int M, int ncols, int K, int n_planes,
                      float *out, int ldc, void *stream);
int dfepe_est_gemm_tn(const void *dY, size_t dy_plane, int Cout, const void *X, size_t x_plane, int Cin, int ncols, int slices,
                      float *part, void *stream);
int dfepe_est_gemm_nt_f16_splitk(const void *A, size_t a_plane, const void *B, size_t b_plane, int M, int ncols, int K,
                                 const unsigned *absmax, float *out, int ldc, int splits, size_t split_stride, void *stream);
int dfepe_est_gemm_nt_splitk(const void *A, size_t a_plane, const void *B, size_t b_plane, int M, int ncols, int K, float *out, int ldc,
                             int splits, size_t split_stride, void *stream);
int dfepe_est_gemm_nt_gx(const void *A, size_t a_plane, const void *B, size_t b_plane, int M, int ncols, int K, float *gx, int C0, int N,
                         long gx_stride_pair, long gx_stride_ch, void *stream);
int dfepe_est_gemm_tn_multi(int n_layers, const void *const *dY, const size_t *dy_plane, const int *Cout, const void *const *X,
                            const size_t *x_plane, const int *Cin, int ncols, const int *slices, float *const *part, void *stream);
int dfepe_est_norm_fwd_r(const float *Y, int ldy, int splits, size_t split_stride, int C, long n_pairs, int N, const float *gamma,
                         const float *beta, float eps, float slope, void *planes_out, size_t out_plane, void *planes_bwd,
                         size_t bwd_plane, float *rstd, void *stream);
int dfepe_est_in_bwd_r(const float *dA, int ldd, int splits, size_t split_stride, const float *dlogit, const float *w_head,
                       const void *planes, size_t plane_stride, const float *rstd, const float *gamma, const float *beta, float slope,
                       int C, long n_pairs, int N, void *dY, size_t dy_plane, float *dgamma_part, float *dbeta_part, void *stream);
size_t dfepe_est_prep_bytes(int n_hidden, const int *Co, const int *Ci);
int dfepe_est_prepare(int n_hidden, const float *const *W, const int *Co, const int *Ci, void *prep, void *stream);
int dfepe_est_dgamma_zero(const float *dA, const float *dlogit, const float *w_head, const void *out_planes, size_t out_plane,
                          const void *in_planes, size_t in_plane, const float *W, int ldw, int Ci, const float *rstd, const float *gamma,
                          float slope, int C, int N, long n_pairs, float *dgamma_part, const void *dY_next, size_t dyn_plane,
                          const float *W_next, int ldw_next, int C_next, void *stream);
int dfepe_est_dgamma_zero_multi(int n_layers, const float *const *dA, const float *const *dlogit, const float *const *w_head,
                                const void *const *out_planes, const size_t *out_plane, const void *const *in_planes,
                                const size_t *in_plane, const float *const *W, const int *Ci, const float *const *rstd,
                                const float *const *gamma, const int *C, float *const *dgamma_part, const void *const *dY_next,
                                const size_t *dyn_plane, const float *const *W_next, const int *C_next, float slope, int N, long n_pairs,
                                void *stream);
int dfepe_est_dgrad_in_bwd(const void *WT, size_t wt_plane, const void *dY_next, size_t dyn_plane, int M, int ncols, int K,
                           const void *aout, size_t aout_plane, const float *rstd, const float *gamma, const float *beta, float slope,
                           void *dY, size_t dy_plane, float *dgamma_part, float *dbeta_part, void *stream);
int dfepe_est_in_bwd(const float *dA, const float *dlogit, const float *w_head, const void *planes, size_t plane_stride,
                     const float *rstd, const float *gamma, const float *beta, float slope, int C, int ncols, void *dY,
                     size_t dy_plane, float *dgamma_part, float *dbeta_part, void *stream);
int dfepe_est_norm_fwd(const float *Y, int ldy, int C, long n_pairs, int N, const float *gamma, const float *beta, float eps,
                       float slope, void *planes_out, size_t out_plane, void *planes_bwd, size_t bwd_plane, float *rstd, int splits,
                       float *part, void *stream);
int dfepe_est_in_bwd_n(const float *dA, const float *dlogit, const float *w_head, const void *planes, size_t plane_stride,
                       const float *rstd, const float *gamma, const float *beta, float slope, int C, long n_pairs, int N, void *dY,
                       size_t dy_plane, float *dgamma_part, float *dbeta_part, int splits, float *part, void *stream);
size_t dfepe_est_saved_bytes(int n_hidden, const int *Co, const int *Ci, long B, int C0, int N, int need_gx);
size_t dfepe_est_forward_workspace_bytes(int n_hidden, const int *Co, const int *Ci, long B, int C0, int N, int keep);
size_t dfepe_est_backward_workspace_bytes(int n_hidden, const int *Co, const int *Ci, long B, int C0, int N, int need_gx);
int dfepe_est_forward(const float *x, long x_stride_b, long x_stride_c, long B, int C0, int N, int n_hidden, const float *const *W, const float *const *gamma,
                      const float *const *beta, const int *Co, const int *Ci, const float *w_head, const float *b_head, float eps,
                      float slope, void *saved, int need_gx, void *workspace, const void *prep, float *logits, void *stream);
int dfepe_est_backward(const float *g_logits, long B, int C0, int N, int n_hidden, const float *const *W, const float *const *gamma,
                       const float *const *beta, const int *Co, const int *Ci, const float *w_head, float slope, const void *saved,
                       void *workspace, const void *prep, float *const *g_W, float *const *g_bias, float *const *g_gamma,
                       float *const *g_beta, float *g_w_head, float *g_b_head, float *gx, long gx_stride_b, long gx_stride_c, void *stream);
int dfepe_est_head_fwd(const void *planes, size_t plane_stride, int C, int ncols, const float *w, const float *bias, float *logits,
                       void *stream);
int dfepe_est_head_dw(const void *planes, size_t plane_stride, int C, int ncols, int blocks, const float *dlogit, float *part,
                      float *bias_part, void *stream);

/*
 * Match construction: what produces the [B,N,4] correspondences of dfepe_w8pt_fwd.
 * Replaces the per-pair host loop of get_matches_from_SP (deepFEPE/train_good_utils.py:683-716):
 *   SP_tracker.nn_match_two_way(desc1.T, desc2.T, nn_thresh)  (:687-691; PointTracker of the un-vendored `superpoint`
 *   package, eric-yyjau/pytorch-superpoint models/model_wrap.py) -> dfepe_nn_match_two_way, batched over the pairs;
 *   xs / offsets / quality gathered through crop_or_pad_choice (:693-716) -> dfepe_gather_matches.
 *
 *   desc1 [B,N1,D], desc2 [B,N2,D]  unit-norm descriptors, fp32, row-major (the reference's pts_desc layout,
 *                                   train_good_utils.py:735), 16-byte aligned; D a multiple of 32 (else UNSUPPORTED)
 *   nn_thresh                       keep a match when its L2 distance sqrt(2 - 2 clip(d1.d2,-1,1)) is < nn_thresh
 *                                   (negative: INVALID_ARG, the reference raises ValueError)
 *   workspace                       dfepe_nn_match_workspace_bytes(B,N1,N2) bytes, 8-byte aligned, contents irrelevant
 *   m_idx1, m_idx2 [B,N1] int32, score [B,N1] fp32: the first count[b] entries of row b are the matches of pair b in
 *                                   increasing m_idx1 order (rows 0,1,2 of the reference's [3,n] array); the rest is
 *                                   not written.   count [B] int32.
 * dmat is never materialised: fp32 MFMA tiles (exact fp32 products, arg-min ties resolved to the first index like
 * numpy.argmin) folded into per-row / per-column minima with 64-bit atomicMin.
 */
size_t dfepe_nn_match_workspace_bytes(int B, int N1, int N2);
int dfepe_nn_match_two_way(const float *desc1, const float *desc2, int B, int N1, int N2, int D, float nn_thresh,
                           void *workspace, int *m_idx1, int *m_idx2, float *score, int *count, void *stream);
/*
 *   pts1 [B,N1,2], pts2 [B,N2,2] keypoints; off1, off2 same shapes (sub-pixel offsets; both NULL with offsets NULL)
 *   choice [B,n_out] int32         positions into the match list of each pair (crop_or_pad_choice, utils_misc.py:139-161;
 *                                   drawn on the host from numpy's RNG like the reference); every value < count[b]
 *   xs [B,n_out,4] = (pts1[m_idx1[c]], pts2[m_idx2[c]]); offsets [B,n_out,4] likewise (may be NULL);
 *   quality [B,n_out] = score[c] (may be NULL)                                   (train_good_utils.py:698-716)
 */
int dfepe_gather_matches(const float *pts1, const float *pts2, const float *off1, const float *off2, int B, int N1, int N2,
                         const int *m_idx1, const int *m_idx2, const float *score, const int *choice, int n_out,
                         float *xs, float *offsets, float *quality, void *stream);

/*
 * Ratio-test 2-NN descriptor matching: the correspondence source of the SIFT-based configs.
 * Replaces the per-pair host call KNN_match (deepFEPE/dsac_tools/utils_opencv.py:39-90, if_BF=True):
 *   cv2.BFMatcher(NORM_L2).knnMatch(des1, des2, k=2)  (:44-45)  and Lowe's ratio test
 *   `m.distance < 0.8 * n.distance`  (:63-67)  -> dfepe_knn_match, batched over the pairs.  The FLANN branch (if_BF=False:
 *   randomised kd-trees, 50 checks) is approximate and not reproducible; this exact search stands in for it too.
 *
 *   desc1 [B,N1,D], desc2 [B,N2,D]  descriptors of any norm, fp32, row-major, 16-byte aligned; D a multiple of 32 (else
 *                                   UNSUPPORTED; SIFT: 128).  NaN components are out of scope.
 *   ratio, ratio_test               ratio_test != 0: row i is good when (double)dist1[i] < ratio * (double)dist2[i], the
 *                                   product in double as Python evaluates the reference's line (NaN ratio: INVALID_ARG);
 *                                   ratio_test == 0: every row is good (if_ratio_test=False) and ratio is ignored
 *   workspace                       dfepe_knn_match_workspace_bytes(B,N1,N2) bytes, 8-byte aligned, contents irrelevant
 *   nn1, nn2 [B,N1] int32           the two columns of desc2 nearest to row i, ordered by (distance, column index): ties keep
 *                                   the lower index first, like OpenCV's k-best insertion (strict < over increasing columns)
 *   dist1, dist2 [B,N1] fp32        their L2 distances: sqrtf of the fp32 squared distance max(|a|^2 + |b|^2 - 2 a.b, 0)
 *   m_idx1, m_idx2 [B,N1] int32, score [B,N1] fp32: the first count[b] entries of row b are the good rows (i, nn1[i], dist1[i])
 *                                   of pair b in increasing i (the reference's good_ij); the rest is not written.  The layout
 *                                   of dfepe_nn_match_two_way: dfepe_gather_matches takes it unchanged.   count [B] int32.
 * all_ij of the reference is (i, nn1[i]) for every i.  N2 < 2 with N1 > 0 has no second neighbour: INVALID_ARG (the reference's
 * `for m, n in matches` raises ValueError).  N1 == 0: count is zeroed, nothing else is written.  B == 0: OK, nothing happens.
 * More than 2^31 - 1 tiles of 128 x 128 over the batch: UNSUPPORTED.  All refusals are made before anything is launched.
 * The distance matrix is never materialised: fp32 MFMA tiles (exact fp32 products), the squared norms accumulated by one fmaf
 * per component in increasing order, t = fma(-2, a.b, |a|^2 + |b|^2); |t - exact| <= (2 D + 3) 2^-23 (max|a|^2 + max|b|^2).
 * Every 64-column strip writes its two best keys per row to its own workspace slot (no atomics, no memset): results do not
 * depend on the launch order and two calls on the same input are bit-identical.
 */
size_t dfepe_knn_match_workspace_bytes(int B, int N1, int N2);
int dfepe_knn_match(const float *desc1, const float *desc2, int B, int N1, int N2, int D, double ratio, int ratio_test,
                    void *workspace, int *nn1, int *nn2, float *dist1, float *dist2, int *m_idx1, int *m_idx2, float *score,
                    int *count, void *stream);

/*
 * Robust fundamental matrix of every pair: OpenCV 3.4 findFundamentalMat(x1, x2, FM_RANSAC, threshold, confidence, max_iters),
 * batched.  Replaces: cv2.findFundamentalMat(x1, x2, cv2.RANSAC, 0.1) in utils_opencv.recover_camera_opencv
 * (deepFEPE/dsac_tools/utils_opencv.py:157), the validation baseline of val_rt (train_good_utils.py:615-633).
 *   matches [B,N,4] fp32 pixels (x1, y1, x2, y2), 16-byte aligned; 15 <= N <= 4096 (N < 15: DFEPE_ERR_UNSUPPORTED -- OpenCV
 *     switches to LMedS there: dfepe_lmeds_fundamental; N > 4096: the pair does not fit in LDS); B <= 65535 (else UNSUPPORTED)
 *   threshold t (pixels, >= 0), confidence p in [0, 1], max_iters >= 1, seed: see the algorithm below
 *   workspace  dfepe_ransac_workspace_bytes(B, N, max_iters) bytes of device memory, 16-byte aligned, overwritten
 *   F_out [B,9] fp32 (F22 = 1; zeros when the pair has no model); inlier_mask [B,N] uint8; n_inliers [B] int32 (0: no model);
 *   iters_run [B] int32 (iterations consumed); best_hyp [B,2] int32 (winning iteration and root, -1 -1 without a model; may be
 *   NULL); hyp_counts [B,max_iters,3] int32 or NULL: the count table (inliers of root r of iteration k; -1 = no such root,
 *   -2 = the iteration drew no sample); masked_matches [B,N,4] or NULL: the matches with every non-inlier row set to quiet NaN
 *   (the `mask=` input of cv2.recoverPose for dfepe_cheirality_ex: a NaN row passes no depth test).
 * The algorithm (sequential definition; the device evaluates all max_iters iterations in parallel and applies this rule to the
 * counts, with the same result):
 *   1 Sampling.  Iteration k draws indices from the stream s_k: draw c is splitmix64(key_k + c * 0x9E3779B97F4A7C15) with
 *     key_k = splitmix64(seed ^ splitmix64(k)), mapped to [0, N) by Lemire's multiply-shift of its upper 32 bits.  The stream
 *     does not depend on the pair (OpenCV re-seeds its RNG with a constant on every call), so a pair's result does not depend on
 *     the batch around it.  7 distinct indices; a sample that fails OpenCV's haveCollinearPoints test for its last point in
 *     either image (|dx2 dy1 - dy2 dx1| <= FLT_EPSILON (|dx1| + |dy1| + |dx2| + |dy2|), non-partial checkSubset) is redrawn from
 *     the same stream; after 1000 attempts the iteration has no sample, the loop ends there, and with k = 0 there is no model.
 *   2 7-point solve in fp64 on the sample normalised per image (centroid 0, RMS distance sqrt(2)): null space {F1, F2} of the
 *     7x9 system with rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] (Householder QR), real roots of
 *     det(l F1 + (1 - l) F2) = 0 ascending (one or three), each F de-normalised and scaled to F22 = 1 where |F22| > DBL_EPSILON.
 *   3 Score: a correspondence is an inlier iff max(d1^2, d2^2) <= t^2 (d2: distance of x2 to the line F x1, d1: of x1 to
 *     F^T x2; OpenCV's FMEstimatorCallback::computeError), evaluated in fp64 on the pixel coordinates without divisions.
 *     Decisions can differ from an exact evaluation only inside a relative band of 1e-6 around t^2.
 *   4 Select: through k = 0, 1, ... and the roots in order, a model whose count exceeds max(best, 6) becomes the best, and
 *     niters = RANSACUpdateNumIters(p, (N - count) / N, 7, niters); the loop stops at k >= niters (niters starts at max_iters).
 *     RANSACUpdateNumIters: num = log(max(1 - p, DBL_MIN)), den = 1 - (1 - ep)^7; den < DBL_MIN: 0; otherwise with
 *     den = log(den): den >= 0 or -num >= niters (-den) ? niters : rint(num / den).
 */
size_t dfepe_ransac_workspace_bytes(int B, int N, int max_iters);
int dfepe_ransac_fundamental(const float *matches, int B, int N, double threshold, double confidence, int max_iters,
                             unsigned long long seed, void *workspace, float *F_out, unsigned char *inlier_mask, int *n_inliers,
                             int *iters_run, int *best_hyp, int *hyp_counts, float *masked_matches, void *stream);
/*
 * Which correspondences the winning pose candidate sees in front of both cameras (cv2.recoverPose's output mask, `mask2` of
 * utils_opencv.recover_camera_opencv, deepFEPE/dsac_tools/utils_opencv.py:177,208).
 *   E, K [B,9]: the matrices handed to dfepe_cheirality_ex (pre = NULL); matches [B,N,4] the same matches (NaN rows: 0), 16-byte
 *   aligned; B <= 65535 (else UNSUPPORTED);
 *   winner [B] its winner output (-1: all zeros); mask [B,N] uint8.
 * The test of every correspondence is the fp64 route of dfepe_cheirality_ex (same rows, normal matrix, eigenvector refinement and
 * depth tests), so the number of ones in a row of mask equals counts[winner] of that call.
 */
int dfepe_ransac_in_front(const float *E, const float *K, const float *matches, int B, int N, float depth_thres, const int *winner,
                          unsigned char *mask, void *stream);

/*
 * Robust essential matrix of every pair by the five-point algorithm: OpenCV 3.4 findEssentialMat(x1, x2, focal, pp, RANSAC,
 * confidence, threshold), batched, in everything but the random stream.  Replaces: cv2.findEssentialMat in
 * utils_opencv.recover_camera_opencv(five_point=True) (deepFEPE/dsac_tools/utils_opencv.py:147-151), the `opencv_5p` baseline of
 * val_rt (train_good_utils.py:615-633).  The pose that follows (cv2.recoverPose, :177) is dfepe_cheirality_ex on E_out itself
 * and masked_matches, with the same K, and dfepe_ransac_in_front.
 *   matches [B,N,4] fp32 pixels (x1, y1, x2, y2), 16-byte aligned; K [B,9] fp32 row-major (K00, K11 the focal lengths, K02, K12
 *     the principal point; nothing else of K is read).  6 <= N <= 4096 (N < 6: DFEPE_ERR_UNSUPPORTED -- with N = 5 OpenCV returns
 *     the stacked models of the one sample, which is not built; N > 4096: the pair does not fit in LDS); B <= 65535 (else
 *     UNSUPPORTED); threshold >= 0 (pixels), confidence p in [0, 1], max_iters >= 1 (else INVALID_ARG); a NULL required pointer
 *     is INVALID_ARG; B == 0 returns 0 before any launch.
 *   workspace  dfepe_ransac5_workspace_bytes(B, N, max_iters) bytes of device memory, 16-byte aligned, overwritten
 *   E_out [B,9] fp32 (the winner, the fp32 rounding of its hyp_E entry; zeros when the pair has no model); inlier_mask [B,N]
 *   uint8; n_inliers [B] int32 (0: no model); iters_run [B] int32 (iterations consumed); best_hyp [B,2] int32 (winning
 *   iteration and root, -1 -1 without a model; may be NULL); hyp_counts [B,max_iters,10] int32 or NULL: the count table
 *   (inliers of root r of iteration k; -1 = no such root; with NULL the table lives in the workspace); hyp_E
 *   [B,max_iters,10,9] fp64 or NULL: the hypotheses themselves, unused slots zero; masked_matches [B,N,4] or NULL: the matches
 *   with every non-inlier row set to quiet NaN.
 * The algorithm (sequential definition; the device evaluates all max_iters iterations in parallel and applies the rule of step
 * 4 to the counts, with the same result):
 *   0 Normalised coordinates in fp64, q = ((x - K02) / K00, (y - K12) / K11) for both images, and the threshold in the same
 *     units, t = threshold / ((K00 + K11) / 2).  With the identity for K the points and the threshold are used as given.
 *   1 Sampling.  The stream of dfepe_ransac_fundamental (same key_k, same Lemire map, independent of the pair); 5 distinct
 *     indices, no geometric rejection: every iteration has a sample, and the table code -2 is never written.
 *   2 Five-point solve in fp64: null space {X, Y, Z, W} of the 5x9 system with rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1,
 *     1] (so that q2^T E q1 = 0 with E row-major; Householder QR), E = x X + y Y + z Z + W, and all real solutions (at most 10)
 *     of det E = 0 and 2 E E^T E - tr(E E^T) E = 0.  Nister's route: the ten cubics as a 10x20 matrix, Gauss-Jordan
 *     elimination with row pivoting, the real roots of the degree-10 determinant in z isolated between the roots of its
 *     derivatives, (x, y) from the null vector, four Gauss-Newton steps on (x, y, z) against the ten constraints.  Each E is
 *     scaled to unit Frobenius norm with its entry of largest magnitude positive; a candidate whose constraints then exceed 1e-9
 *     is not a solution and is dropped.  The solutions of an iteration are in ascending z: a function of the sample alone.
 *   3 Score: a correspondence is an inlier iff (q2^T E q1)^2 <= t^2 ((E q1)_0^2 + (E q1)_1^2 + (E^T q2)_0^2 + (E^T q2)_1^2), the
 *     Sampson error of OpenCV's EMEstimatorCallback::computeError, evaluated in fp64 without divisions.  Decisions can differ
 *     from an exact evaluation only inside a relative band of 1e-6 around t^2.
 *   4 Select: the rule of dfepe_ransac_fundamental with 10 slots per iteration: a model whose count exceeds max(best, 4) becomes
 *     the best, and niters = RANSACUpdateNumIters(p, (N - count) / N, 5, niters) (den = 1 - (1 - ep)^5).
 */
size_t dfepe_ransac5_workspace_bytes(int B, int N, int max_iters);
int dfepe_ransac_essential(const float *matches, const float *K, int B, int N, double threshold, double confidence,
                           int max_iters, unsigned long long seed, void *workspace, float *E_out,
                           unsigned char *inlier_mask, int *n_inliers, int *iters_run, int *best_hyp,
                           int *hyp_counts, double *hyp_E, float *masked_matches, void *stream);

/*
 * Least-median-of-squares fundamental and essential matrix of every pair: OpenCV 3.4's LMeDSPointSetRegistrator::run, batched.
 * Replaces: what cv2.findFundamentalMat(x1, x2, cv2.RANSAC, 0.1) (deepFEPE/dsac_tools/utils_opencv.py:157) runs on a pair with
 * fewer than 15 correspondences -- OpenCV does not run RANSAC there but LMedS, and no threshold is used -- and
 * cv2.findEssentialMat(.., method=LMEDS), which is what recover_camera_opencv(five_point=True, RANSAC=False) (:137-151) means in
 * OpenCV.  The pose that follows is dfepe_cheirality_ex on masked_matches and dfepe_ransac_in_front, as for the RANSAC entries.
 *   matches [B,N,4] fp32 pixels (x1, y1, x2, y2), 16-byte aligned; K [B,9] fp32 as for dfepe_ransac_essential.
 *     Fundamental: 8 <= N <= 4096 (N = 7 is OpenCV's direct 7-point path, not built); essential: 6 <= N <= 4096; outside:
 *     DFEPE_ERR_UNSUPPORTED; B <= 65535 (else UNSUPPORTED); confidence p in [0, 1], max_iters >= 1 (else INVALID_ARG); a NULL
 *     required pointer is INVALID_ARG; B == 0 returns 0 before any launch.  m = 7 (fundamental) or 5 (essential) below.
 *   dfepe_lmeds_num_iters(m, p, max_iters): niters of step 1 (negative: INVALID_ARG); it sizes hyp_medians.
 *   workspace  dfepe_lmeds_workspace_bytes(B, m, p, max_iters) bytes of device memory, 16-byte aligned, overwritten
 *   F_out / E_out [B,9] fp32 (the winning root as the RANSAC entries scale it; zeros when the pair has no model); inlier_mask
 *   [B,N] uint8; n_inliers [B] int32 (0: no model); iters_run [B] int32 (iterations the loop went through); best_hyp [B,2] int32
 *   (winning iteration and root, -1 -1 without a model; may be NULL); min_median [B] fp64 (DBL_MAX when no median was finite;
 *   may be NULL); sigma [B] fp64 (0 when no median was finite; may be NULL); hyp_medians [B,niters,3] resp. [B,niters,10] fp64 or
 *   NULL: the median table (median of root r of iteration k, an fp32 value or +inf; -1 = no such root, -2 = the iteration drew no
 *   sample; with NULL the table lives in the workspace); masked_matches [B,N,4] or NULL: the matches with every non-inlier row
 *   set to quiet NaN.
 * The algorithm (sequential definition; the device evaluates all niters iterations in parallel and applies the rule of step 5 to
 * the medians, with the same result):
 *   1 niters = RANSACUpdateNumIters(p, 0.45, m, max_iters) (the rule of dfepe_ransac_fundamental resp. dfepe_ransac_essential),
 *     fixed for the whole run: 300 for p = 0.99, m = 7.  There is no adaptive update.  niters = 0 (p = 0): no model.
 *   2 Iteration k samples and solves exactly as the RANSAC entry of the same m does: the same stream and key_k, for m = 7 the
 *     same collinearity redraw (no sample at k = 0: no model; at k > 0: the loop ends there), the same 7-point resp. five-point
 *     solve (for m = 5 on the normalised coordinates of dfepe_ransac_essential step 0): up to 3 resp. 10 models.
 *   3 The error of every correspondence under every model, evaluated in fp64 and rounded to fp32: for F max(d1^2, d2^2) in px^2
 *     with the divisions by the line norms (d2: distance of x2 to F x1, d1: of x1 to F^T x2); for E the Sampson error
 *     (q2^T E q1)^2 / ((E q1)_0^2 + (E q1)_1^2 + (E^T q2)_0^2 + (E^T q2)_1^2) in normalised coordinates.  A zero denominator or a
 *     non-finite value counts as +inf.
 *   4 Median: the fp32 errors sorted ascending (by their bit patterns as integers: valid for non-negative floats); odd N:
 *     sorted[N/2]; even N: (sorted[N/2 - 1] + sorted[N/2]) * 0.5 with the sum in fp32.
 *   5 Select: through k = 0, 1, ... and the roots in order, a model becomes the best when its median is strictly below
 *     minMedian, which starts at DBL_MAX: an infinite median never wins.
 *   6 sigma = max(2.5 * 1.4826 * (1 + 5 / (N - m)) * sqrt(minMedian), 0.001); a correspondence is an inlier when its fp32 error
 *     is <= (float)(sigma^2).  Fewer than m inliers: no model (zeros, best_hyp = -1 -1, n_inliers = 0; min_median and sigma keep
 *     their values).  There is no refit.
 * What differs from OpenCV: the random stream (as for the RANSAC entries), and the errors are the fp32 rounding of an fp64
 * evaluation, not a float evaluation, so near-ties between two medians can fall the other way.  OpenCV also replaces a confidence
 * outside (0, 1) by 0.99 before it starts; here 0 and 1 are taken as given.
 * The median is a selection, not a sort: one wavefront per model holds the N errors in ceil(N / 64) registers per lane and finds
 * the rank-N/2 pattern from the most significant bit down (31 rounds of a per-lane count and a wavefront sum).  No atomics: two
 * calls on the same input are bit-identical, and a pair's result does not depend on the batch around it.
 * dfepe_version() stays 154 with this addition: the number is pinned by existing tests, and nothing that existed changes.
 */
int dfepe_lmeds_num_iters(int model_points, double confidence, int max_iters);
size_t dfepe_lmeds_workspace_bytes(int B, int model_points, double confidence, int max_iters);
int dfepe_lmeds_fundamental(const float *matches, int B, int N, double confidence, int max_iters, unsigned long long seed,
                            void *workspace, float *F_out, unsigned char *inlier_mask, int *n_inliers, int *iters_run,
                            int *best_hyp, double *min_median, double *sigma, double *hyp_medians, float *masked_matches,
                            void *stream);
int dfepe_lmeds_essential(const float *matches, const float *K, int B, int N, double confidence, int max_iters,
                          unsigned long long seed, void *workspace, float *E_out, unsigned char *inlier_mask, int *n_inliers,
                          int *iters_run, int *best_hyp, double *min_median, double *sigma, double *hyp_medians,
                          float *masked_matches, void *stream);

/*
 * Optimal correction of correspondences onto a given epipolar geometry (Hartley & Sturm), batched: for every pair (p, q) the pair
 * (p', q') with q'^T F p' = 0 exactly that minimises |p - p'|^2 + |q - q'|^2 -- cv2.correctMatches(F, p, q), OpenCV's argument
 * order.  Replaces: the cv2.correctMatches call of get_virt_x1x2_np / get_virt_x1x2 (deepFEPE/dsac_tools/utils_misc.py:176,206),
 * which makes the virtual points pts*_virt_ori of the F-loss once per sample on the host.
 *   stream comes first here (a hipStream_t, as everywhere).
 *   F [B,9] fp64 row-major with f_stride = 9, or one F [9] for all pairs with f_stride = 0 (any other stride: INVALID_ARG).
 *     F is fp64 because its rounding to fp32 moves the result by more than one fp32 spacing at pixel scale.
 *   p, q [B,M,2] fp32 pixels; p_out, q_out [B,M,2] fp32; cost [B,M] fp32 or NULL: the minimal |p - p'|^2 + |q - q'|^2 in px^2.
 *   B < 0, M < 0: INVALID_ARG; B == 0 or M == 0 returns 0 before any launch; then a NULL required pointer is INVALID_ARG; more
 *   than 2^31 - 1 workgroups of 256 points: UNSUPPORTED.
 * One lane per point, everything in fp64:
 *   1 the epipoles e1 (F e1 = 0), e2 (e2^T F = 0): the largest cross product of two rows / two columns of F (scaled by max |F|);
 *   2 p and q are translated to the origins, the translated epipoles scaled to ex^2 + ey^2 = 1 and rotated onto (1, 0, f1),
 *     (1, 0, f2); of the transformed F only a = G11, b = G12, c = G21, d = G22 remain;
 *   3 the real roots of the sextic t ((a t + b)^2 + f2^2 (c t + d)^2)^2 - (a d - b c) (1 + f1^2 t^2)^2 (a t + b) (c t + d)
 *     (Hartley & Zisserman eq. 12.7; coefficients divided by the largest), those with |t| <= 1 in t and those with |t| >= 1 in
 *     u = 1 / t: in either chart the roots in [-1, 1] are bracketed by the roots of the derivative, level by level from the linear
 *     fifth derivative, and every bracket with a sign change gets 36 halvings and 3 Newton steps;
 *   4 the cost s(t) = t^2 / (1 + f1^2 t^2) + (c t + d)^2 / ((a t + b)^2 + f2^2 (c t + d)^2) at every root and at t = infinity; the
 *     smallest wins, its closest points (t^2 f1, t, t^2 f1^2 + 1) and (f2 (c t + d)^2, -(a t + b)(c t + d), f2^2 (c t + d)^2 +
 *     (a t + b)^2) are rotated and translated back and rounded to fp32.
 *   A point on an epipole (ex^2 + ey^2 = 0) and any lane whose result is not finite get quiet NaN in all five outputs, as OpenCV
 *   returns NaN there.
 * dfepe_version() stays 154 with this addition: the number is pinned by existing tests, and nothing that existed changes.
 */
int dfepe_correct_matches(void *stream, const double *F, long f_stride, const float *p, const float *q, int B, int M, float *p_out,
                          float *q_out, float *cost);

/*
 * Odometry evaluation, part 1: relative poses -> trajectory.  Replaces Exp_table_processor.get_abs_poses
 * (deepFEPE/utils/eval_tools.py:268-284: last = pose @ last; abs.append(inv(last)[:3]); the identity first) and, with cam2body,
 * the camera-to-body conjugation in front of it (relative_pose_cam_to_body, Train_model_pipeline.py:1098-1108:
 * inv(Rt_cam2_gt) @ M @ Rt_cam2_gt, collected as relative_poses_body at :1110-1119).  Everything is fp64; a pose is a 3x4 affine
 * map, row-major, with the implied last row (0, 0, 0, 1).
 *   stream comes first (a hipStream_t).
 *   rel [S,n_max,12]: the relative poses P_1 .. P_n of each sequence; lengths [S] int32 or NULL (every sequence has n_max poses);
 *     a length is clamped to [0, n_max].
 *   cam2body: NULL, or [S,n_max,12] with c2b_stride = 12 (one per pose), or [S,12] with c2b_stride = 0 (one per sequence); any
 *     other stride is INVALID_ARG.  With it P_k is replaced by inv(C) P_k C (general inverse, evaluated left to right).
 *   abs_out [S,n_max+1,12]: entry 0 is the identity, entry k is inv(P_k ... P_1) -- the general inverse (adjugate over
 *     determinant, then -A^-1 t), not the transpose, as numpy.linalg.inv in the reference.  Entries past lengths[s] are not
 *     written.
 *   S < 0, n_max < 0: INVALID_ARG; S == 0 returns 0 before any launch; then a NULL abs_out, or a NULL rel with n_max > 0, is
 *   INVALID_ARG; n_max >= 2^31 / 12 - 1: UNSUPPORTED.
 * One workgroup of 256 lanes per sequence, tiles of 256 x 8 poses: every lane composes its 8 consecutive poses in order, the lane
 * totals are scanned with wavefront shuffles and the wavefront totals through LDS (the later operand always on the left), and every
 * lane walks its poses again from its prefix, inverts and stores.  No atomics, no dependence on arrival order: the result is the
 * same bits on every run, and its first 8 entries are those of the sequential loop.  Floating-point contraction is off in this
 * code (csrc/odometry_math.h says why).
 */
int dfepe_pose_chain(void *stream, const double *rel, const int *lengths, const double *cam2body, long c2b_stride, int S, int n_max,
                     double *abs_out);

/*
 * Odometry evaluation, part 2: the snippet ATE / RE.  Replaces Exp_table_processor.pose_seq_ate (eval_tools.py:334-375) with its
 * compensate_poses (:252-265) and compute_pose_error (:309-331), as notebooks/exp_process_table.ipynb calls it
 * (pose_seq_ate(poses_abs_tmp, poses_gt, 5)).  fp64 throughout; the errors are rounded to fp32 because the reference's array is.
 *   est, gt [S,m_max,12] absolute poses; windows [S] int32: the number of windows of each sequence, window w covering poses
 *     w .. w + L - 1.  The reference scores len(est) - L windows -- it never scores the last one -- so that is what its mirror
 *     passes; 1 scores a single snippet.  windows[s] + L - 1 <= the number of valid poses of sequence s is the CALLER's
 *     contract: it cannot be checked without a synchronisation (the value is clamped to [0, min(W, m_max - L + 1)], so nothing is
 *     read or written outside the buffers, but poses past a sequence's own length are the caller's padding).
 *   W: the window capacity of the outputs; L = seq_length, 1 <= L <= 64 (anything else: UNSUPPORTED).
 *   no_compensate != 0: the poses are scored as given (a stand-alone compute_pose_error); 0: each window of est and of gt first
 *     goes through compensate_poses: the window's first translation is subtracted from every translation, then every pose, all
 *     four columns, is multiplied from the left by the general inverse of the window's first 3x3.
 *   compute_pose_error is called as (est_snip, gt_snip) on parameters named (gt, pred), so:
 *     scale = sum(est_t . gt_t) / sum(gt_t^2);  ATE = |est_t - scale gt_t| / L;
 *     RE = (sum_i atan2(|(R01 - R10, R12 - R21, R02 - R20)|, tr R - 1)) / L,  R = est_R inv(gt_R).
 *     Ground-truth translations that are all zero give NaN / inf as numpy does.
 *   errors [S,W,2] fp32 (ATE, RE); scale [S,W] fp64; aligned [S,W,12] fp64: est[w] as given with its translation times scale;
 *   compensated [S,W,L,12] fp64 or NULL: the compensated estimate of every window (with no_compensate: the window as given);
 *   rows w >= windows[s] are not written.  stats [S,4] fp64: (ATE mean, ATE std, RE mean, RE std), the mean and the population
 *   standard deviation of the fp32-rounded errors of the sequence's windows, two passes in a fixed order (each lane its own
 *   windows ascending, then a binary tree over the lanes), no atomics; NaN for a sequence without windows.
 *   S, m_max, W < 0: INVALID_ARG; S == 0 returns 0 before any launch; then NULL windows or stats, and with W > 0 NULL est, gt,
 *   errors, scale or aligned, are INVALID_ARG.  (S > 0 with W == 0 still launches: it writes the NaN statistics.)
 * One workgroup per sequence, one lane per window.
 */
int dfepe_snippet_errors(void *stream, const double *est, const double *gt, const int *windows, int S, int m_max, int W, int L,
                         int no_compensate, float *errors, double *scale, double *aligned, double *compensated, double *stats);

/*
 * KITTI odometry table, part 1: first-frame re-basing and trajectory alignment (the published KITTI devkit / kitti-odom-eval
 * evaluation, steps 1 and 2).  fp64 throughout; poses as in dfepe_pose_chain.
 *   est, gt [S,n_max,12] absolute poses; est_len, gt_len [S] int32 or NULL (n_max).  n = gt_len clamped to [0, n_max] and
 *     m = est_len clamped to [0, n]: frame i of the estimate belongs to frame i of the ground truth, and nothing is read or written
 *     past m resp. n.
 *   Every pose is re-based on its trajectory's first one, inv(P_0) P_i (general inverse).  Then, with x the estimate's and y the
 *   ground truth's translations over the m common frames, mode is
 *     DFEPE_TRAJ_NONE        nothing more;
 *     DFEPE_TRAJ_SCALE       c = sum x.y / sum x.x, the estimate's translations times c;
 *     DFEPE_TRAJ_SCALE_7DOF, DFEPE_TRAJ_7DOF, DFEPE_TRAJ_6DOF   Umeyama: means, sigma_x^2 = (1/m) sum |x - mx|^2 and
 *       C = (1/m) sum (y - my)(x - mx)^T in two passes (means first, then centred sums), C = U D V^T (3x3 one-sided Jacobi),
 *       S = diag(1, 1, -1) when det(U) det(V^T) < 0, r = U S V^T, c = tr(D S) / sigma_x^2 (1 for 6DOF), t = my - c r mx.
 *       SCALE_7DOF multiplies the estimate's translations by c only; 7DOF and 6DOF multiply them by c and then every pose from the
 *       left by [r | t].  sigma_x^2 = 0 gives the IEEE result of the formula (inf or NaN), which propagates.  A planar trajectory
 *       (C of rank 2) is decided: the column of U of the smallest singular value is the cross product of the other two.  A
 *       collinear trajectory leaves r and t undetermined (NaN or no rotation); c, and with it SCALE_7DOF, is still decided.
 *   est_out, gt_out [S,n_max,12]: the aligned estimate (m poses) and the re-based ground truth (n poses); not the inputs' memory.
 *   rtc [S,13]: r (9, row-major), t (3), c; the identity, 0 and 1 where a mode does not compute them (and for m = 0).
 *   S < 0, n_max < 0 or an unknown mode: INVALID_ARG; S == 0 returns 0 before any launch; then a NULL rtc, or with n_max > 0 a NULL
 *   est, gt, est_out or gt_out, is INVALID_ARG; n_max >= 2^31 / 12 - 1: UNSUPPORTED.
 * One workgroup of 256 lanes per sequence; every sum is a fixed tree (a lane's frames ascending, a butterfly across the wavefront,
 * the wavefront totals in order).  No atomics: the same bits on every run.  Contraction is off (csrc/odometry_math.h says why).
 */
#define DFEPE_TRAJ_NONE 0
#define DFEPE_TRAJ_SCALE 1
#define DFEPE_TRAJ_SCALE_7DOF 2
#define DFEPE_TRAJ_7DOF 3
#define DFEPE_TRAJ_6DOF 4
int dfepe_trajectory_align(void *stream, const double *est, const double *gt, const int *est_len, const int *gt_len, int S, int n_max,
                           int mode, double *est_out, double *gt_out, double *rtc);

/*
 * KITTI odometry table, part 2: segment errors, ATE and RPE of aligned trajectories (steps 3 to 5 of the same evaluation).
 *   est, gt [S,n_max,12], est_len, gt_len: as above (the outputs of dfepe_trajectory_align).
 *   dist [S,n_max] fp64: written; dist[i] = the ground truth's path length up to frame i.
 *   For first = 0, step, 2 step, ... < n and len = 100, 200, .. 800: last = the first i >= first with dist[i] > dist[first] + len,
 *   found by bisection; the pair is scored unless there is no such i, or last >= m, or first >= m.  (dist is a parallel scan:
 *   where the ground truth stands still dist[i + 1] can round a few last places below dist[i], and the bisection can then place
 *   last differently from a linear search only where dist is within that rounding of dist[first] + len.)  With
 *   E = inv(inv(est_first) est_last) (inv(gt_first) gt_last), r = arccos(clamp((tr E_R - 1) / 2, -1, 1)), t = |E_t|:
 *   rows [S,F,8,5] fp64: [first, r / len, t / len, len, len / (0.1 (last - first + 1))], zeros for a pair that is not scored;
 *   valid [S,F,8] bytes: 1 scored, 0 not; F >= ceil(n_max / step), so that the rows hold every first frame (fewer: INVALID_ARG);
 *   rows of first frames >= n are not written.  count [S] int32: scored pairs.
 *   summary [S,5] fp64: t_rel = 100 mean(t / len) in %, r_rel = mean(r / len) 180 / pi 100 in deg / 100 m (both 0 without a scored
 *   pair, as the devkit), ATE = sqrt(mean_i |gt_xyz,i - est_xyz,i|^2) over the m frames (NaN for m = 0), and the RPE over i < m - 1
 *   with E = inv(inv(gt_i) gt_i+1) (inv(est_i) est_i+1): mean |E_t| in m and mean angle in degrees (NaN for m <= 1).
 *   S < 0, n_max < 0, step < 1, F < 0: INVALID_ARG; S == 0 returns 0 before any launch; then NULL count or summary, with n_max > 0
 *   NULL est, gt or dist, with F > 0 NULL rows or valid, are INVALID_ARG; n_max >= 2^31 / 12 - 1 or F > (2^31 - 1) / 40: UNSUPPORTED;
 *   then F step < n_max: INVALID_ARG.
 * One workgroup per sequence: a shuffle-and-LDS scan for dist (kept in LDS up to 4096 frames, read from `dist` beyond), one lane per
 * (first, len) pair, lanes striding the frames for ATE and RPE, one fixed-order reduction.  No atomics; the same bits on every run.
 */
int dfepe_kitti_odometry_errors(void *stream, const double *est, const double *gt, const int *est_len, const int *gt_len, int S,
                                int n_max, int step, int F, double *dist, double *rows, unsigned char *valid, int *count,
                                double *summary);

/*
 * Two-view structure: the 3-D points and depths that the pose kernels reduce to one bit each, and the projection back.
 * Common rules: B < 0 or N < 0 (M < 0), an unknown flag bit, a stride other than 0 (one matrix for all pairs) or the row size
 * (12 for a 3x4, 9 for K): INVALID_ARG; then B == 0 or N == 0 returns 0 before any launch; then a required pointer that is NULL,
 * or matches (and Xh, which is written as float4 too) not 16-byte aligned: INVALID_ARG; then B > 65535: UNSUPPORTED.  All of
 * it is decided on the host before any HIP call.  One launch per call, one lane per correspondence, no host synchronisation, no
 * allocation, nothing written outside the stated extents; a non-finite row touches only its own outputs.
 *
 * dfepe_triangulate: cv2.triangulatePoints for B pairs.
 *   P1, P2 3x4 fp32 projection matrices (stride 0 or 12); matches [B,N,4] pixels (x1, y1, x2, y2); Xh [B,N,4] fp32.
 *   Per correspondence Xh is the unit 2-norm null vector (last right singular vector) of the 4x4 matrix
 *     A = [x1 P1_3 - P1_1; y1 P1_3 - P1_2; x2 P2_3 - P2_1; y2 P2_3 - P2_2]      (P_i: row i; the published DLT),
 *   computed in fp64 from the fp32 inputs (one-sided Jacobi on A itself, csrc/triangulate_math.h) and rounded once, with the sign
 *   w = Xh[3] >= 0 (OpenCV leaves the sign to its SVD; every call site divides by w).  Scaling both matrices by the same power of
 *   two changes no bit.  A non-finite match row, a non-finite matrix or A = 0 give four NaNs for that row only.
 *   Accuracy (tests/triangulate_ref.py): with s1 >= .. >= s4 the singular values of A and
 *     eta = max(1e-8, 64 2^-52 s1^2 / (s3^2 - s4^2)),  |Xh - Xh_ref|_inf <= eta + 2^-24 wherever eta is finite.
 *
 * dfepe_two_view_structure: the points and depths of a pose's correspondences (DeepFNet.get_depth after cv2.recoverPose).
 *   Rt [B,3,4] fp32: scene motion (x2 ~ R x1 + t), or with DFEPE_POSE_CAMERA_MOTION camera motion -- what dfepe_cheirality_ex
 *   writes -- whose inverse R = Rc^T, t = -Rc^T tc (utils_misc._inv_Rt) is formed in fp64.  K [B,3,3] fp32.  Cameras P1 = K [I | 0],
 *   P2 = K [R | t] in fp64, the triangulation above, then X = Xh[:3] / w in the frame of camera 1, z1 = X[2], z2 = (R X + t)[2],
 *   all fp64 up to one rounding.  scale [B] or NULL multiplies X, z1 and z2 (the reference's t_scene_scale: a recovered t has unit
 *   norm).  clamp > 0 clamps z1 and z2, after scaling, to [-clamp, clamp] (torch.clamp(tri_depths * t_scene_scale, -150., 150.),
 *   DeepFNetSampleLoss.py:614); X is not clamped; NaN stays NaN.  winner [B] int32 or NULL: a pair with winner < 0 has no pose and
 *   gets NaN rows.  X [B,N,3], z1, z2 [B,N] fp32: each may be NULL, all three NULL is INVALID_ARG.  w = 0 gives what the fp64
 *   division gives (inf or NaN); it never traps.
 *
 * dfepe_reproject: the numeric part of dsac_tools/utils_vis.reproj_and_scatter.
 *   X [B,M,3] fp32; Rt (stride 0 or 12) and flags as above; K (stride 0 or 9).  u = K (R X + t) in fp64 from the fp32 inputs,
 *   x [B,M,2] = (u0 / u2, u1 / u2) and z [B,M] = u2 rounded once; inside [B,M] bytes = (x >= 0) & (y >= 0) & (x <= image_w) &
 *   (y <= image_h) evaluated on the fp32 values written to x (utils_misc.within with xlim = im_shape[1], ylim = im_shape[0]):
 *   NaN gives 0, and there is no depth test, as in the reference.  z and inside may be NULL.
 */
#define DFEPE_POSE_CAMERA_MOTION 1u   /* Rt is camera motion (what dfepe_cheirality_ex writes); scene motion is R = Rc^T, t = -Rc^T tc, as utils_misc._inv_Rt */

int dfepe_triangulate(const float *P1, int p1_stride, const float *P2, int p2_stride, const float *matches, int B, int N, float *Xh,
                      void *stream);
int dfepe_two_view_structure(const float *Rt, unsigned flags, const float *K, const float *matches, int B, int N, const int *winner,
                             const float *scale, float clamp, float *X, float *z1, float *z2, void *stream);
int dfepe_reproject(const float *X, const float *Rt, int rt_stride, unsigned flags, const float *K, int k_stride, int B, int M,
                    float image_w, float image_h, float *x, float *z, unsigned char *inside, void *stream);

/*
 * Robust homography of every pair: OpenCV 3.4 findHomography(x1, x2, RANSAC, threshold, maxIters, confidence), batched.
 * Replaces: cv2.findHomography(m_keypoints, m_warped_keypoints, cv2.RANSAC) in evaluations/descriptor_evaluation.py:93-95
 * (compute_homography) and in deepFEPE/evaluate_frontend.py:234-236 (getInliers_cv).
 *   matches [B,N,4] fp32 pixels (x1, y1, x2, y2), 16-byte aligned; 1 <= N <= 4096 (N < 1: INVALID_ARG; N > 4096: UNSUPPORTED, the
 *     pair does not fit in LDS); B <= 65535 (else UNSUPPORTED); B == 0 returns OK
 *   n_valid [B] int32 or NULL: pair b uses its first n = clamp(n_valid[b], 0, N) rows (cross-checked matches differ in number from
 *     pair to pair); rows past n get mask 0; NULL means N for every pair
 *   threshold t in pixels; t <= 0 means 3 (cv2's rule); NaN: INVALID_ARG.  confidence p in [0, 1], max_iters >= 1 (else INVALID_ARG)
 *   flags: DFEPE_HOMOGRAPHY_ALL_POINTS is cv2's method = 0: no sampling, the mask is all ones, the model is step 6 over all n
 *     points, then step 7.  DFEPE_HOMOGRAPHY_NO_REFINE skips step 7, so H_out is the refit.  Any other bit: INVALID_ARG
 *   workspace  dfepe_homography_workspace_bytes(B, N, max_iters) bytes of device memory, 16-byte aligned, overwritten
 *   H_out [B,9] fp64 (cv2 returns float64), H[8] = 1, zeros when the pair has no model; H_model [B,9] fp64 or NULL: the winning
 *     sample's H before the refit (with ALL_POINTS: the result of step 6); inlier_mask [B,N] uint8; n_inliers [B] int32 (0: no
 *     model); iters_run [B] int32 (iterations consumed; 0 where nothing is sampled); best_iter [B] int32 or NULL (-1 without a
 *     sampled winner); hyp_counts [B,max_iters] int32 or NULL: the count table (-1 = the sample gave no model, -2 = no sample,
 *     also every entry of a pair with n <= 4; not written with ALL_POINTS)
 *   All refusals are made before anything is launched.  No atomics; every cell has one writer; two calls on the same input are
 *   bit-identical; no host synchronisation, no allocation.
 * The algorithm (sequential definition; the device evaluates all max_iters iterations in parallel and applies the rule to the
 * counts, with the same result).  OpenCV is not available where this was written and its results are not pinned by golden
 * vectors: what follows is the definition, held to the fp64 restatement tests/homography_ref.py; only the random stream is ours.
 *   0 Pair sizes.  n < 4: no model.  n = 4: one solve (step 2) on the four points, mask all ones, no sampling, no refinement.
 *     A pair without a model gives H = 0, mask 0 and n_inliers = 0.
 *   1 Sampling.  The stream of dfepe_ransac_fundamental (same key_k, same Lemire map, independent of the pair), 4 distinct indices.
 *     A sample is redrawn from the same stream when the non-partial checkSubset fails: the last point is collinear with two
 *     earlier ones in either image (the test of dfepe_ransac_fundamental), or the orientation test fails -- over the triples
 *     {0,1,2}, {0,1,3}, {0,2,3}, {1,2,3} the number with det[src_i 1] det[dst_i 1] < 0 (each det of the 3x3 matrix of rows
 *     (x, y, 1), in fp64 from the fp32 coordinates) must be 0 or 4.  After 1000 attempts the iteration has no sample.
 *   2 4-point solve (runKernel) in fp64: per image the centroid c and the per-axis sums s = sum |x - c|; any s < FLT_EPSILON: no
 *     model; scales n / s.  With the normalised source (X, Y) and target (x, y) each point gives the rows
 *     (X, Y, 1, 0, 0, 0, -xX, -xY, -x) and (0, 0, 0, X, Y, 1, -yX, -yY, -y).  For the minimal sample h is the null vector of the
 *     8x9 system taken directly: Householder QR of its transpose, the last column of Q (not the eigenvector of L^T L; the
 *     restatement's second route takes the SVD).  H = T_dst^-1 H0 T_src scaled so that H[8] = 1; H[8] zero or not finite before
 *     the scaling: no model.
 *   3 Score: err = ((H00 x + H01 y + H02)/w - x')^2 + ((H10 x + H11 y + H12)/w - y')^2 with w = H20 x + H21 y + 1; inlier iff
 *     err <= t^2, evaluated in fp64 without divisions: (X - x'w)^2 + (Y - y'w)^2 <= t^2 w^2; w = 0 is never an inlier.
 *   4 Select: the rule of dfepe_ransac_fundamental with one slot per iteration and 4 model points: a model whose count exceeds
 *     max(best, 3) becomes the best, niters = RANSACUpdateNumIters(p, (n - count)/n, 4, niters), the loop stops at k >= niters or
 *     at the first iteration without a sample.
 *   5 Mask: the winner's inliers by step 3.  It is not recomputed after steps 6 and 7 (OpenCV keeps the RANSAC mask).
 *   6 Refit, when n > 4 and a model was found: runKernel over all inliers of the winner in its n-point form -- centroids, scales,
 *     the 9x9 L^T L accumulated in fp64, the eigenvector of its smallest eigenvalue by cyclic Jacobi, de-normalised as in 2.
 *     When this gives no model the winner's H stays (OpenCV ignores the return value); with ALL_POINTS the pair then has none.
 *   7 Refinement: Levenberg-Marquardt, at most 10 iterations, on h[0..7] with h[8] = 1, over the inliers, in pixels.
 *     Residuals r = (X/w - x', Y/w - y') with 1/w := 0 where |w| <= DBL_EPSILON.  Set-up: A = J^T J, v = J^T r, D = diag(A) taken
 *     once, S = |r|^2, lambda = 1, lc = 0.75.  Each iteration:
 *       a solve (A + lambda diag(D)) d = v by the symmetric eigen decomposition Q diag(e) Q^T (cyclic Jacobi); an eigenvalue with
 *         |e_i| <= 2 DBL_EPSILON sum_j |e_j| is treated as zero (its direction contributes nothing to d);
 *       b x_d = x - d;  S_d = |r(x_d)|^2;  dS = d^T (2 v - A d);  R = (S - S_d) / (|dS| > DBL_EPSILON ? dS : 1);
 *       c R > 0.75: lambda *= 0.5, then lambda = 0 if lambda < lc;
 *         else R < 0.25: nu = clamp((S_d - S) / (|d^T v| > DBL_EPSILON ? d^T v : 1) + 2, 2, 10); if lambda = 0:
 *         lambda = lc = 1 / max(DBL_EPSILON, max_i |(A^-1)_ii|) (A^-1 by the same decomposition and zero rule) and nu *= 0.5;
 *         lambda *= nu;
 *       d S_d < S: accept, x = x_d, and r, J, A, v, S are recomputed;
 *       e stop after 10 iterations, or when |d|_inf < FLT_EPSILON, or when |r|_inf < FLT_EPSILON (r of the kept x).
 *     This loop is a restatement of OpenCV's LMSolver from memory; what is written here is the definition.
 *
 * dfepe_homography_transfer: evaluate_frontend.getInliers (deepFEPE/evaluate_frontend.py:210-228).  H [B,9] fp64; matches and
 *   n_valid as above (N >= 0; B == 0 or N == 0: OK, nothing happens); dist [B,N] fp32 = |H x1 - x2| (the fp64 value of
 *   sqrt(dx^2 + dy^2) after the division by w, rounded once; w = 0 gives what the division gives), mask [B,N] uint8 = dist < epi
 *   on the fp64 value, with the reference's strict <.  Rows past n_valid get dist 0 and mask 0.  dist or mask may be NULL, not both.
 * dfepe_homography_corners: the correctness test of descriptor_evaluation.compute_homography (lines 104-123).  H_est, H_gt
 *   [B,9] fp64; the corners (0,0), (0,height-1), (width-1,0), (width-1,height-1) are warped by both, mean_dist [B] fp64 (or NULL)
 *   is the mean of the four distances, correct [B,T] uint8 = mean_dist <= thresh[j] for the T thresholds in device memory
 *   (thresh [T] fp64).  height, width >= 1, T >= 0 (T == 0: only mean_dist).  An all-zero H_est (no model) gives NaN and 0.
 */
#define DFEPE_HOMOGRAPHY_ALL_POINTS 1u /* cv2's method = 0: least squares over all points, then the refinement */
#define DFEPE_HOMOGRAPHY_NO_REFINE 2u  /* no Levenberg-Marquardt step: H_out is the refit */

size_t dfepe_homography_workspace_bytes(int B, int N, int max_iters);
int dfepe_ransac_homography(const float *matches, const int *n_valid, int B, int N, double threshold, double confidence,
                            int max_iters, unsigned long long seed, unsigned flags, void *workspace, double *H_out,
                            double *H_model, unsigned char *inlier_mask, int *n_inliers, int *iters_run, int *best_iter,
                            int *hyp_counts, void *stream);
int dfepe_homography_transfer(const double *H, const float *matches, const int *n_valid, int B, int N, double epi, float *dist,
                              unsigned char *mask, void *stream);
int dfepe_homography_corners(const double *H_est, const double *H_gt, int B, int height, int width, const double *thresh, int T,
                             double *mean_dist, unsigned char *correct, void *stream);

/*
 * The rest of the reference's front-end table (deepFEPE/evaluate_frontend.py:45: correctness, repeatability, localization_err,
 * mscore, mAP; correctness is dfepe_homography_corners), batched over B image pairs.  All arithmetic and all floating-point
 * arguments are fp64.  No atomics; every output cell has one writer and every sum a fixed order, so two calls on the same input
 * are bit-identical; no host synchronisation, no allocation; all refusals are made before anything is launched, in the order
 * in which they are listed.
 *
 * dfepe_keypoint_repeatability: compute_repeatability (evaluations/detector_evaluation.py:150-279).
 *   kp1 [B,N1,C], kp2 [B,N2,C]: rows (x, y[, prob]) of image 1 (data['prob']) and image 2 (data['warped_prob']); C is 2 or 3
 *   n1, n2 [B] int32 or NULL: pair b uses its first clamp(n[b], 0, N) rows; NULL means all.  H [B,9], image 1 to image 2
 *   height, width >= 1: data['image'].shape.  keep_k >= 0: keep_k_points.  thresh [T] in device memory, T >= 0 (T == 0: only
 *   kept1, kept2 and n_unwarped are written; the other outputs may then be NULL)
 *   workspace: dfepe_keypoint_repeatability_workspace_bytes(B, N1, N2) bytes of device memory, 16-byte aligned, overwritten
 *   repeatability, loc_err [B,T] fp64; count1, count2 [B,T] int32; kept1, kept2, n_unwarped [B] int32
 *   Refused: B, N1, N2, T or keep_k < 0, C not 2 or 3, height or width < 1: INVALID_ARG.  Then B == 0 returns OK.  N1 or N2 >
 *   4096, or B > 65535: UNSUPPORTED.  A null kp1 with N1 > 0 (kp2, N2 alike), a null H, kept1, kept2 or n_unwarped; with T > 0 a
 *   null thresh or [B,T] output; with N1 + N2 > 0 a null or misaligned workspace: INVALID_ARG.
 *   The definition:
 *   1 Image-2 points are warped by adj(H) (transposed cofactors: the same projective map as inv(H), no division by the
 *     determinant) and kept when the warp lies in 0 <= x < width, 0 <= y < height (keep_true_keypoints); the kept points keep
 *     their own coordinates.  n_unwarped counts the image-2 points whose warp lies in 0 <= x <= width - 1, 0 <= y <= height - 1,
 *     both ends inclusive, nothing truncated: the warpLabels count of the matching score, stated here because that helper's
 *     package is not part of the reference's tree.
 *   2 Image-1 points are warped by H and the warped points kept under the half-open test (filter_keypoints).  A point whose
 *     homogeneous w is 0 gives what the division gives, and fails both tests through the comparisons themselves.
 *   3 select_k_best, with C = 3: of each kept set the min(keep_k, n) points that stand last in a stable ascending argsort of the
 *     probabilities, that is the largest, and among equal probabilities the higher index (numpy's default argsort, which the
 *     reference calls, is not stable: there the choice among equals at the k-th place is undefined).  NaN sorts above +inf,
 *     -0 equals +0, as in numpy.  min(keep_k, n) = 0 keeps every point, as numpy's [-0:] does.  With C = 2 nothing is selected.
 *     kept1, kept2: the sizes N1, N2 after this step.
 *   4 min1[i]: the Euclidean distance from kept point i of image 1 (warped) to the nearest kept point of image 2, min2 the same
 *     with the roles swapped.  count1[t] = #{min1 <= thresh[t]} (not strict), 0 when kept2 = 0; count2 alike.
 *   5 repeatability = (count1 + count2) / (kept1 + kept2); loc_err = sum(counted min1) / (count1 + count2) + sum(counted min2) /
 *     (count1 + count2); 0 and -1 when nothing is counted.  The reference overwrites its caller's data['prob'][:, :2] with the
 *     warped points (line 228); nothing here writes to an input.
 *
 * dfepe_average_precision: sklearn.metrics.average_precision_score(labels, scores), evaluate_frontend.py:244-275.
 *   labels [B,M] uint8 (non-zero: positive), scores [B,M]; n_valid [B] int32 or NULL as above.  ap [B]; n_pos [B] int32 or NULL;
 *   tp_at, cnt_at [B,M] int32 or NULL (each on its own); cells past n_valid get 0.
 *   Refused: B or M < 0: INVALID_ARG.  B == 0 returns OK.  M > 4096 or B > 65535: UNSUPPORTED.  A null ap, or with M > 0 null
 *   labels or scores: INVALID_ARG.
 *   scikit-learn's value groups tied scores; it equals   AP = (1/P) sum over positives i of TP(s_i) / CNT(s_i)   with
 *   TP(s) = #{j: score_j >= s, label_j = 1} = tp_at, CNT(s) = #{j: score_j >= s} = cnt_at, P = #positives = n_pos: no sort, no
 *   dependence on the order of equal scores, exact in its integer parts.  ap = 0 for a pair without a valid entry or without a
 *   positive (evaluate_frontend.py:268-273).  A NaN score is at least as high as nothing: its cnt_at is 0, and the ap of a pair
 *   with a NaN-scored positive is NaN.
 *
 * dfepe_matching_score: evaluate_frontend.py:181.  mscore[b] = 2 n_inliers[b] / (n_kp1[b] + n_unwarped[b]) (all [B] int32, the
 *   last from dfepe_keypoint_repeatability); a zero denominator gives what the division gives.  B < 0 or (with B > 0) a null
 *   pointer: INVALID_ARG; B == 0 returns OK.
 */
size_t dfepe_keypoint_repeatability_workspace_bytes(int B, int N1, int N2);
int dfepe_keypoint_repeatability(const double *kp1, const double *kp2, const int *n1, const int *n2, const double *H, int B, int N1,
                                 int N2, int C, int height, int width, int keep_k, const double *thresh, int T, void *workspace,
                                 double *repeatability, double *loc_err, int *count1, int *count2, int *kept1, int *kept2,
                                 int *n_unwarped, void *stream);
int dfepe_average_precision(const unsigned char *labels, const double *scores, const int *n_valid, int B, int M, double *ap, int *n_pos,
                            int *tp_at, int *cnt_at, void *stream);
int dfepe_matching_score(const int *n_inliers, const int *n_kp1, const int *n_unwarped, int B, double *mscore, void *stream);

/*
 * The SuperPoint output processing of the end-to-end training path: process_SP_output (deepFEPE/train_good_utils.py:727-755),
 * batched over B images.  Its steps are methods of the superpoint package (superpoint.models.model_utils.SuperPointNet_process,
 * superpoint.utils), which the reference's tree does not hold: what follows is the published algorithm, unpinned, and this text
 * is its specification.  Data are fp32, the arithmetic of every value is fp64 and is rounded once.  No atomics; every cell has one
 * writer and every sum a fixed order, so two calls on the same input are bit-identical; no host synchronisation, no allocation;
 * all refusals are made before anything is launched, in the order in which they are listed.  H, W: the image in pixels; a cell is
 * 8 x 8 pixels, (Hc, Wc) = (H/8, W/8).  Limits: H * W <= 2^24 pixels per image, patch_size <= 63; beyond: UNSUPPORTED.
 *
 * dfepe_sp_flatten: flattenDetection after set_nan2zero (train_good_utils.py:741-743, models/model_utils.py:5-15).
 *   semi [B,65,Hc,Wc]; a NaN is read as 0.  heatmap [B,1,H,W] (16-byte aligned): the softmax over the 65 channels without channel
 *   64 (the dustbin); channel c of cell (hc, wc) is pixel (8 hc + c/8, 8 wc + c%8).
 *   Refused: B < 0, H or W < 1 or not a multiple of 8: INVALID_ARG.  H * W beyond the limit: UNSUPPORTED.  Then B == 0 returns OK.
 *   A null semi, a null or misaligned heatmap: INVALID_ARG.
 * dfepe_sp_flatten_bwd: its adjoint.  g_heatmap [B,1,H,W] -> g_semi [B,65,Hc,Wc], all 65 channels written:
 *   g_semi[c] = p_c (g_c - sum_{k<64} g_k p_k) with g_64 = 0, so the dustbin receives its share through the normaliser; 0 where
 *   semi is NaN (the 0 it was read as is a constant).  Refusals as above (null semi, g_heatmap or g_semi: INVALID_ARG).
 *
 * dfepe_sp_nms: heatmap_to_nms (train_good_utils.py:745), the greedy nms_fast, for any input.
 *   heatmap [B,1,H,W]; candidates are the pixels with h >= conf_thresh (a NaN is none).  nms_dist = d >= 0, border_remove = r >= 0.
 *   Candidates are visited by confidence descending and, among equal confidences, row-major index ascending (a stated rule: the
 *   reference's argsort is not stable).  A candidate is kept iff no candidate kept before it lies within Chebyshev distance d.
 *   After that a kept point with x < r, x >= W - r, y < r or y >= H - r is removed: it has still suppressed its neighbours.
 *   nms_map [B,1,H,W]: 1.0 at the kept points, 0.0 elsewhere (heatmap_to_nms(tensor=True)).  cap = dfepe_sp_nms_capacity(H, W, d) =
 *   ceil(H/(d+1)) ceil(W/(d+1)) (0 for arguments that dfepe_sp_nms refuses): two kept points never share a (d+1) x (d+1) block, so
 *   the list cannot overflow, and a constant heatmap reaches cap.  pts [B,cap,2] int32 (x, y) in row-major order of the pixels
 *   (the order of nonzero()), conf [B,cap] their heat, count [B] int32; entries from count[b] on are 0.
 *   workspace: dfepe_sp_nms_workspace_bytes(B, H, W) bytes of device memory, overwritten: 0 (NULL allowed) up to H * W = 12288
 *   pixels, where heat and state stay in LDS, else five bytes per pixel (a state byte, the B planes together rounded up to 16,
 *   then an int32 list of the pixels still undecided when the one-workgroup loop takes over).
 *   Refused: B < 0, H or W < 1, d < 0, r < 0: INVALID_ARG.  Then B == 0 returns OK.  H * W beyond the limit or B > 65535:
 *   UNSUPPORTED.  A null heatmap, nms_map, pts, conf or count, a null workspace where one is needed: INVALID_ARG.
 *   The loop runs on the device as a fixpoint without a round limit: every candidate starts undecided; an undecided candidate
 *   becomes suppressed when a kept candidate that outranks it lies in its window, kept when every candidate in its window that
 *   outranks it is suppressed; it ends when none is undecided (DESIGN.md 3.15 shows that this is the greedy loop's result).
 *   One workgroup per image loops on a workgroup-wide test; above the LDS size four rounds over the whole device come first.
 *
 * dfepe_sp_soft_argmax: pred_soft_argmax (train_good_utils.py:747).
 *   pts, count: a point list as dfepe_sp_nms writes it (image b uses its first clamp(count[b], 0, cap) rows).  patch_size = p, odd,
 *   1 <= p <= 2 border_remove + 1, so that the p x p patch h centred on a listed point lies inside the image (a row whose patch
 *   does not is treated as not listed).  q = h / (sum h + 1e-6); q < 0 -> 1e-6; l = log q; e = exp(l - max l);
 *   off_x = sum x e / (sum e + 1e-6) - p/2 (integer division) with x = 0..p-1 the column, off_y alike with the row.  A patch with
 *   sum h <= 0 gives (0, 0) and no gradient (a stated rule: the formulas give NaN).  pred [B,cap,2] (x, y), 0 for rows not listed;
 *   patches [B,cap,p,p] or NULL: q after the clamp.
 *   Refused: B < 0, H or W < 1, cap < 0, r < 0, p < 1, p even, p > 2r + 1: INVALID_ARG.  H * W beyond the limit, p > 63 or B * cap >=
 *   2^31: UNSUPPORTED.  Then B == 0 or cap == 0 returns OK.  A null heatmap, pts, count or pred: INVALID_ARG.
 * dfepe_sp_soft_argmax_bwd: g_pred [B,cap,2] -> g_heatmap [B,1,H,W], written whole.  The exact derivative of the formulas above,
 *   the maximum's share included and spread evenly over the entries that attain it; nothing flows through a clamped entry.  In
 *   gather form: each pixel sums, in row-major window order, what the listed points whose patch covers it send, so overlapping
 *   patches (p > d) are bit-identical from run to run.  workspace: dfepe_sp_soft_argmax_bwd_workspace_bytes(B, H, W, cap) bytes,
 *   16-byte aligned, overwritten (a dense int32 map of list positions and one record per listed point).
 *   Refusals as the forward's; then B == 0 returns OK; a null heatmap or g_heatmap, a null or misaligned workspace, with cap > 0 a
 *   null pts, count or g_pred: INVALID_ARG.
 *
 * dfepe_sp_sample_desc: sample_desc_from_points (train_good_utils.py:750, inside batch_extract_features).
 *   desc [B,D,Hc,Wc]; positions pts + pred in pixels (pred NULL: pts alone).  Normalised coordinates x / (W/2) - 1, y / (H/2) - 1;
 *   bilinear sampling with zero padding, grid_sample's rule for align_corners (1 is what the torch version that the reference pins,
 *   1.3.1, did; 0 is today's default); the sample is divided by its L2 norm over D, a zero norm gives zeros (a stated rule).
 *   out [B,cap,D], zero rows from count[b] on.  Forward only: the reference detaches these descriptors (train_good_utils.py:664).
 *   Refused: B < 0, D < 1, H or W < 1 or not a multiple of 8, cap < 0, align_corners not 0 or 1: INVALID_ARG.  Then B == 0 or cap == 0
 *   returns OK.  H * W beyond the limit or B > 65535: UNSUPPORTED.  A null desc, pts, count or out: INVALID_ARG.
 *
 * dfepe_gather_offsets_bwd: the adjoint of the offsets output of dfepe_gather_matches (train_good_utils.py:700-711) into off1 and
 *   off2.  g_offsets [B,n_out,4] -> g_off1 [B,N1,2], g_off2 [B,N2,2], written whole.  Padding repeats choices, so rows collide: one
 *   lane per source keypoint adds the rows that name it in ascending row order, in fp64.
 *   Refused: B < 0, N1 or N2 < 1, n_out < 0: INVALID_ARG.  Then B == 0 returns OK.  B > 65535: UNSUPPORTED.  A null g_off1, g_off2,
 *   m_idx1 or m_idx2, with n_out > 0 a null g_offsets or choice: INVALID_ARG.
 */
int dfepe_sp_nms_capacity(int H, int W, int nms_dist);
size_t dfepe_sp_nms_workspace_bytes(int B, int H, int W);
size_t dfepe_sp_soft_argmax_bwd_workspace_bytes(int B, int H, int W, int cap);
int dfepe_sp_flatten(const float *semi, int B, int H, int W, float *heatmap, void *stream);
int dfepe_sp_flatten_bwd(const float *semi, const float *g_heatmap, int B, int H, int W, float *g_semi, void *stream);
int dfepe_sp_nms(const float *heatmap, int B, int H, int W, float conf_thresh, int nms_dist, int border_remove, void *workspace,
                 float *nms_map, int *pts, float *conf, int *count, void *stream);
int dfepe_sp_soft_argmax(const float *heatmap, const int *pts, const int *count, int B, int H, int W, int cap, int patch_size,
                         int border_remove, float *pred, float *patches, void *stream);
int dfepe_sp_soft_argmax_bwd(const float *heatmap, const int *pts, const int *count, const float *g_pred, int B, int H, int W, int cap,
                             int patch_size, int border_remove, void *workspace, float *g_heatmap, void *stream);
int dfepe_sp_sample_desc(const float *desc, const int *pts, const float *pred, const int *count, int B, int D, int H, int W, int cap,
                         int align_corners, float *out, void *stream);
int dfepe_gather_offsets_bwd(const float *g_offsets, int B, int N1, int N2, const int *m_idx1, const int *m_idx2, const int *choice,
                             int n_out, float *g_off1, float *g_off2, void *stream);

/*
 * The correspondence evaluation (run_eval_good.py --runCorr, :380-384 -> evaluation_epiDist.py val_feature), batched over B image
 * pairs: the epipolar distance of every match under the ground-truth F (epi_dist_from_matches, deepFEPE/evaluation_epiDist.py:
 * 276-326 -> val_rt -> epi_distance_np, deepFEPE/dsac_tools/utils_F.py:363-385) and Result_processor's table of inlier ratios by
 * match score (deepFEPE/utils/eval_tools.py:27-174: inlier_ratio :70-104, get_mask :145-147, inlier_ratio_nested :151-162,
 * inlier_ratio_from_est :164-174; ap_inlier_thd :113-137 sweeps the mask threshold; Exp_table_processor.get_result_dict :423-429
 * calls inlier_ratio with mask_thd = 1.0).  No atomics of any kind; every output cell has one writer, so two calls on the same
 * input are bit-identical; no host synchronisation, no allocation; all refusals are made before anything is launched, in the order
 * in which they are listed.  dfepe_version() stays 154 with this addition: the number is pinned by existing tests, and nothing that
 * existed changes.
 *
 * dfepe_inlier_table: one launch, one 256-thread workgroup per pair.
 *   matches [B,N,4] fp32 (x1, y1, x2, y2; 16-byte aligned) with F [B,9] fp64 row-major, OR dist [B,N] fp32 (a distance computed
 *     before): exactly one of matches and dist (with N == 0 neither is read and both may be NULL)
 *   scores [B,N] fp32 or NULL (no mask: every match is kept; then Tm must be 1 and mask_thds is not read and may be NULL)
 *   n_valid [B] int32 or NULL: pair b uses its first clamp(n_valid[b], 0, N) rows, as in dfepe_ransac_homography; NULL means all
 *   inlier_thds [Ti], mask_thds [Tm] fp64 in device memory, 1 <= Ti, Tm <= 16
 *   outputs, each may be NULL but not all of them:
 *     cnt [B,Tm,Ti] int32   #{i: score_i < mask_thds[m] and dist_i < inlier_thds[t]}
 *     num [B,Tm] int32      #{i: score_i < mask_thds[m]}                       (inlier_ratio's num_corrs)
 *     ratio [B,Tm,Ti] fp64  (double)cnt / (double)num: 0 / 0 = NaN for a pair with nothing kept, as inlier_ratio_from_est gives
 *     dist_out [B,N] fp32   the distance rounded once; rows past n_valid are 0
 *   The distance is dist3 of epi_distance_np, in fp64 from the fp32 coordinates widened exactly, by the reference's sequence
 *   (csrc/corr_eval_math.h spells out every association; no fused multiply-add):
 *     a = y^T F;  nominator = |a . x|;  p = (F x)_12;  q = (F^T y)_12;  dist3 = nominator * (1 / sqrt(p.p) + 1 / sqrt(q.q))
 *   with x = (x1, y1, 1), y = (x2, y2, 1).  The reciprocals come first, so F x = 0 gives 0 * inf = NaN where numpy gives it and a
 *   non-zero numerator over a zero norm gives +inf.  Both comparisons are strict `<` in fp64 (the score widened to fp64, the
 *   distance compared before it is rounded for dist_out; a dist input is widened to fp64).  A NaN passes neither test: a NaN
 *   score is not kept; a kept match with a NaN distance is no inlier and stays in the denominator, as in numpy.
 *   Refused: B or N < 0, Ti or Tm outside 1 .. 16, both matches and dist given, scores NULL with Tm != 1: INVALID_ARG.  Then
 *   B == 0 returns OK and nothing is written.  With N > 0 neither matches nor dist; matches without F or not 16-byte aligned; a
 *   null inlier_thds; scores with a null mask_thds; all four outputs NULL: INVALID_ARG.  N == 0 (or a pair with nothing valid)
 *   is launched like any other: cnt and num 0, ratio NaN.
 *
 * dfepe_inlier_table_mean: one launch, one workgroup.
 *   ratio [B,Tm,Ti] fp64 and num [B,Tm] int32 as written above -> mean [Tm,Ti] fp64 = the sum over the pairs in index order
 *   (b = 0, 1, ...: the order of numpy's table.mean(axis=0)), divided by B; a NaN ratio makes the mean NaN, B == 0 gives 0 / 0 =
 *   NaN.  num_T [Tm,B] int32 = num transposed, the layout ap_inlier_thd returns.  Either output may be NULL, not both.
 *   Refused: B < 0, Ti or Tm outside 1 .. 16, both outputs NULL, with B > 0 a null ratio with mean or a null num with num_T:
 *   INVALID_ARG.  B == 0 is launched (mean is NaN).
 */
int dfepe_inlier_table(const float *matches, const double *F, const float *dist, const float *scores, const int *n_valid, int B, int N,
                       const double *inlier_thds, int Ti, const double *mask_thds, int Tm, int *cnt, int *num, double *ratio,
                       float *dist_out, void *stream);
int dfepe_inlier_table_mean(const double *ratio, const int *num, int B, int Tm, int Ti, double *mean, int *num_T, void *stream);

/*
 * Adjoints of the epipolar distances (csrc/epi_adjoint.hip, csrc/epi_adjoint_math.h): the gradients of dfepe_epi_metrics with
 * respect to F, X and Y, the gradient of the epipolar residual with respect to its points, and the reduced loss sum_n w e with its
 * adjoint.  The reference's _sym_epi_dist, _sampson_dist, _epi_distance and compute_epi_residual (deepFEPE/dsac_tools/utils_F.py:
 * 291-361, 400-413) are plain torch and so differentiable in every argument; get_loss_softmax (train_good_utils.py:55-61), HLoss
 * (dsac_tools/H_loss.py) and the soft inlier count of dsac_tools/dsac.py rely on that.  fp32 in and out, fp64 inside, every output
 * rounded once.  No atomics, no allocation, no host synchronisation: the calls can be captured in a hipGraph, and a pair's result is
 * the same bits on every run and whatever else is in the batch.  dfepe_version() stays 154 with this addition: the number is pinned
 * by existing tests, and nothing that existed changes.
 *
 * `kind`, DFEPE_EPI_HOMOGENEOUS, `clamp_at` (< 0: no clamp; kind 0 only) and `eps` mean what they mean for dfepe_epi_metrics.  With
 * x = (x0, x1, x2) and y likewise (third coordinate the constant 1, without a gradient, unless DFEPE_EPI_HOMOGENEOUS), a = F x,
 * b = F^T y, s = y^T F x, A = a0^2 + a1^2, Q = b0^2 + b1^2:
 *   kind 0   e = s^2 (1/(A+eps) + 1/(Q+eps)) =: s^2 R    de = 2 s R ds - s^2 (dA/(A+eps)^2 + dQ/(Q+eps)^2), where e <= clamp_at
 *            (torch.clamp(max=) passes the gradient AT the bound), 0 elsewhere
 *   kind 1   e = s^2 / (A+Q)                             de = 2 s ds/(A+Q) - s^2 (dA+dQ)/(A+Q)^2
 *   kind 2   d1 = |s|/sqrt(A), d2 = |s|/sqrt(Q), planes ((d1+d2)/2, d1, d2); the three upstream planes g_out [3,B,N] are combined
 *            per point; dd1 = sign(s) ds/sqrt(A) - |s| dA/(2 A^(3/2)), dd2 likewise; sign(0) = 0
 *   ds/dF_rc = y_r x_c, ds/dx = b, ds/dy = a;  dA/dF_rc = 2 a_r x_c [r<2], dA/dx_c = 2 (a0 F_0c + a1 F_1c);
 *   dQ/dF_rc = 2 b_c y_r [c<2], dQ/dy_r = 2 (b0 F_r0 + b1 F_r1).
 * A point whose forward value is not finite (F x = 0 with eps = 0, a NaN input) may produce anything in its own g_X, g_Y (g_w) rows
 * and in its own pair's g_F (sum); it changes no bit of any other pair's outputs or of any other point's rows.
 *
 * Launch shape: a workgroup of 256 lanes owns a chunk of P = dfepe_epi_adjoint_chunk() consecutive points of one pair.  The nine
 * fp64 partial sums of g_F (the one of the loss) are reduced in a fixed order: per lane, across the wavefront, the four wavefront
 * totals in order.  With N <= P the workgroup writes the result and there is one launch; otherwise its doubles go to `workspace`
 * [B, ceil(N/P), 9] (dfepe_epi_adjoint_workspace_bytes(B, N) bytes, 8-byte aligned, contents irrelevant) and a second launch on the
 * same stream adds the chunks in ascending order.  The workspace is only touched for g_F and for the loss sum.
 *
 * Refusals, made on the host before any HIP call, in this order: B or N < 0, a kind outside 0..2 (| DFEPE_EPI_HOMOGENEOUS), or
 * clamp_at >= 0 on kinds 1 and 2: INVALID_ARG.  Then B == 0 or N == 0 returns OK: nothing is launched and nothing written.  A NULL
 * input, every output NULL, [B,N,2] points or point gradients that are not 8-byte aligned, a NULL or misaligned workspace when it
 * is needed (N > P and g_F or the sum asked for): INVALID_ARG.  B * N > 2^31 - 1: UNSUPPORTED (the grid has B * ceil(N/P) blocks).
 *
 * dfepe_epi_metrics_bwd: g_out [B,N] (kinds 0, 1) or [3,B,N] (kind 2) -> g_F [B,9], g_X, g_Y [B,N,2|3]; an output that is NULL is
 *   skipped (for g_F the sums and the second launch too); whichever are asked for, each has the same bits.
 * dfepe_epi_residual_bwd_pts: compute_epi_residual w.r.t. its points (w.r.t. F: dfepe_epi_residual_bwd).  pts1, pts2 [B,N,3], F
 *   [B,9], g_out [B,N] -> g_pts1, g_pts2 [B,N,3] (either may be NULL).  With l1 = F^T x2, l2 = F x1, dd = x2^T F x1, n = |l[:2]|,
 *   i = 1/(n + 1e-6), S = i1 + i2, d = |dd| S:  dd/dx1 = sign(dd) S l1 - k2 F[:2,:]^T l2[:2],  dd/dx2 = sign(dd) S l2 -
 *   k1 F[:,:2] l1[:2],  k = |dd| i^2 / n (0 where n = 0); the gradient passes where d <= clamp_at; sign(0) = 0.
 * dfepe_epi_loss_fwd: sum_out [B] = sum_n w[b,n] e[b,n] (w [B,N] or NULL = 1); e is kind 0 or 1, or the first plane of kind 2.
 *   The per-point values are never written.
 * dfepe_epi_loss_bwd: g_sum [B] -> g_F, g_X, g_Y as above with the upstream g_sum[b] w[b,n], and g_w [B,N] = g_sum[b] e[b,n]
 *   (recomputed); each may be NULL, not all.
 */
int dfepe_epi_adjoint_chunk(void);
size_t dfepe_epi_adjoint_workspace_bytes(int B, int N);
int dfepe_epi_metrics_bwd(void *stream, int kind, const float *F, const float *X, const float *Y, int B, int N, float clamp_at,
                          float eps, const float *g_out, float *g_F, float *g_X, float *g_Y, void *workspace);
int dfepe_epi_residual_bwd_pts(void *stream, const float *pts1, const float *pts2, const float *F, int B, int N, float clamp_at,
                               const float *g_out, float *g_pts1, float *g_pts2);
int dfepe_epi_loss_fwd(void *stream, int kind, const float *F, const float *X, const float *Y, const float *w, int B, int N,
                       float clamp_at, float eps, float *sum_out, void *workspace);
int dfepe_epi_loss_bwd(void *stream, int kind, const float *F, const float *X, const float *Y, const float *w, int B, int N,
                       float clamp_at, float eps, const float *g_sum, float *g_F, float *g_X, float *g_Y, float *g_w, void *workspace);

/*
 * DSAC: the hypothesis loop of deepFEPE/dsac_tools/dsac.py (class DSAC, :138-176, :194) for B pairs and H hypotheses each, in six
 * launches whatever B and H are (csrc/dsac.hip, csrc/dsac_math.h).  The reference runs it on the CPU, one hypothesis at a time
 * ("working on CPU because of many, small matrices", :110).  fp32 in and out, fp64 inside, every output rounded once.  No atomics,
 * no allocation, no host synchronisation: the call can be captured in a hipGraph (one linear chain of launches), and a pair's
 * outputs are the same bits on every run and whatever else is in the batch.  dfepe_version() stays 154 with this addition: the
 * number is pinned by existing tests, and nothing that existed changes.
 *
 *   X, Y [B,N,2] pixel points, 8-byte aligned; K [B,9]
 *   idx  [B,H,S] int32: the S correspondences sampled for each hypothesis (random.sample(range(N), 10), :46: S = 10), 8 <= S <= 16,
 *        N >= S.  Contract, not checked on the device: 0 <= idx < N, and the indices of one hypothesis are distinct.  (An index
 *        outside 0..N-1 is clamped into the pair by the sample fit and matches no correspondence in the vote.)
 *   loss_kind  0: none (loss = 0).  1: HLoss(E_refit, X, Y), the mean Sampson distance of the PIXEL points under E_refit itself,
 *        as :157 with H_loss.py:28 computes it.  2: the same under F = K^-T E_refit K^-1.
 * Stages:
 *   1 sample fit (:37-52)   E_sample [B,H,9] = _E_from_XY of the S sampled correspondences: K^-1 points with _de_homo's 1e-10 guard
 *     (utils_F.py:111-112, rounded to fp32), then dfepe_w8pt_fwd with DFEPE_W8PT_SQRT2 | NO_ROWNORM | FORCE_110 on B H problems.
 *   2 soft inlier count (:56-76)   F = K^-T E_sample K^-1 (utils_F._E_to_F; the reference names an undefined E_to_F) from the fp32
 *     E_sample, d = _sampson_dist(F, X, Y) on the pixel points, soft = 1 / (1 + exp(beta (d - thresh))) (= 1 - sigmoid(.), :72),
 *     score = sum_n soft in fp64 in a fixed order (lane l adds n = l, l + 64, ...; the 64 partial sums by a balanced tree).
 *     sampson, soft [B,H,N] (each may be NULL), score [B,H].
 *   3 refit (:78-92, :150)  E_refit [B,H,9] = _E_from_XY of all N correspondences with the row weights sqrt(soft), soft as written
 *     (fp32); the Hartley transforms are unweighted.  dfepe_w8pt_fwd with n_weight_sets = H.
 *   4 loss (:157)           loss [B,H] according to loss_kind, from the fp32 E_refit, summed in the order of stage 2.
 *   5 vote (:163-175, :194) counts [B,N] (float32) = the number of hypotheses that sampled the correspondence, quality [B,N] =
 *     N_scores / (N_counts + 1e-10) in float32, N_scores = the float32 scores added in hypothesis order: bit-identical to the
 *     reference's sequential `+=` given the scores.  best [B] int32 = the first hypothesis whose score is the strict maximum above
 *     0 (:130, :168), -1 when no score is above 0 (a NaN score is never above).  The step the reference leaves commented out
 *     (:178-190): exp_loss [B] = sum_h softmax(alpha score)_h loss_h, top_loss [B] = loss[best] (0 when best = -1); each may be NULL.
 * The sign of E_sample and E_refit is dfepe_w8pt_fwd's gauge; every other output is sign-invariant.  A non-finite input stays in its
 * own pair.
 *   workspace: dfepe_dsac_workspace_bytes(B, N, H, S) bytes, 16-byte aligned, contents irrelevant (the K^-1 points, the gathered
 *     samples, the refit's weights [H,B,N], the residuals the fits write, E_refit as the fit lays it out [H,B,9]).
 *   dfepe_dsac_hyps_per_block(): hypotheses of one pair per workgroup in launches 3 and 5 (a wavefront each);
 *   dfepe_dsac_vote_chunk(): consecutive correspondences of one pair per workgroup in the vote;
 *   dfepe_dsac_vote_tile(): hypotheses whose index lists that workgroup stages in LDS at a time.
 * Refusals, made on the host before any HIP call, in this order: B or N < 0, H < 1, S outside 8..16, N < S, loss_kind outside 0..2:
 * INVALID_ARG.  Then B == 0 returns OK: nothing is launched and nothing written.  A NULL X, Y, K, idx, E_sample, score, E_refit,
 * loss, quality, counts, best or workspace; X or Y not 8-byte aligned; a workspace that is not 16-byte aligned: INVALID_ARG.
 * B * H * N > 2^31 - 1: UNSUPPORTED.  The adjoint of the loop is dfepe_dsac_bwd below, the device-side sampler that fills idx on the
 * stream is dfepe_sample_sets at the end of this header.  Not built: losses other than the two above.
 */
int dfepe_dsac_hyps_per_block(void);
int dfepe_dsac_vote_chunk(void);
int dfepe_dsac_vote_tile(void);
size_t dfepe_dsac_workspace_bytes(int B, int N, int H, int S);
int dfepe_dsac(void *stream, const float *X, const float *Y, const float *K, const int *idx, int B, int N, int H, int S,
               float inlier_thresh, float inlier_beta, float inlier_alpha, int loss_kind, float *E_sample, float *soft, float *sampson,
               float *score, float *E_refit, float *loss, float *quality, float *counts, int *best, float *exp_loss, float *top_loss,
               void *workspace);

/*
 * Adjoint of the textbook normalised eight-point solvers: utils_F._F_from_XY (deepFEPE/dsac_tools/utils_F.py:223-275), _E_from_XY
 * (:104-155) and _E_from_XY_batch (:157-221), i.e. of dfepe_w8pt_fwd with DFEPE_W8PT_SQRT2 | DFEPE_W8PT_NO_ROWNORM, which
 * dfepe_w8pt_bwd refuses (csrc/eight_point_adjoint.hip, csrc/eight_point_adjoint_math.h).  Gradients to the points and the weights.
 * fp32 in and out, fp64 inside, every output rounded once.  Nothing is saved by the forward: the fit is recomputed.  No atomics, no
 * allocation, no host synchronisation: the call (at most two launches) can be captured in a hipGraph, and a problem's outputs are the
 * same bits on every run and whatever else is in the batch.  A non-finite input stays in its own pair.  dfepe_version() stays 154 with
 * this addition: the number is pinned by existing tests, and nothing that existed changes.
 *
 *   X, Y   [B,N,2]  the 2-D points the forward saw (its third coordinate was 1), 8-byte aligned; N >= 8
 *   w      [S,B,N]  or NULL (= 1); S = n_weight_sets >= 1, the forward's layout
 *   flags  must contain DFEPE_W8PT_SQRT2 | DFEPE_W8PT_NO_ROWNORM; DFEPE_W8PT_FORCE_110 and DFEPE_W8PT_NO_HARTLEY are optional
 *   F_out  [S,B,9]  the forward's output: only its sign is read, the recomputed matrix is oriented to it by their inner product
 *   g_F    [S,B,9]  the gradient w.r.t. F_out as given
 *   g_X, g_Y [B,N,2] (8-byte aligned), g_w [S,B,N]: written, not accumulated; each may be NULL and is then skipped, not all three.
 *          With S > 1, g_X[b,n] and g_Y[b,n] are the sums over the weight sets, added in set order in fp64.
 *   workspace  dfepe_eight_point_bwd_workspace_bytes(B, N, S) bytes, 16-byte aligned, contents irrelevant; 0 bytes (NULL allowed)
 *          when S == 1; only touched when S > 1 and g_X or g_Y is asked for.
 *
 * Per problem (pair b, weight set s), with p~ the normalised points (c = mean p, scale = sqrt(2) / mean |p - c|,
 * p~ = scale (p - c) / (1 + 1e-10), T = [[scale,0,-scale cx],[0,scale,-scale cy],[0,0,1]]; p~ = p, T = I with NO_HARTLEY):
 *   a_i = [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1], A_i = w_i a_i, M9 = A^T A = sum lam_k q_k q_k^T, f = q_9 (smallest),
 *   F0 = reshape(f) = U diag(s1,s2,s3) V^T, M = U diag(s1,s2,0) V^T (FORCE_110: diag(1,1,0)), out = T2^T M T1.
 * T1 and T2 are CONSTANTS in the adjoint: the reference builds them with torch.tensor([[S1, 0, ...]]) (utils_F.py:25,35, and :52,65
 * in the batch form), which detaches them, so the reference's own gradient never passes through the centroid or the scale.
 *   G = T2 g_F T1^T, G^ = U^T G V, g_F0 = U P V^T, d_k = s_k^2 - s3^2 (k = 1, 2):
 *     without FORCE_110 (M = F0 - s3 u3 v3^T):  P = G^ except P_33 = 0, P_k3 = G^_k3 + s3 (s3 G^_k3 + s_k G^_3k) / d_k,
 *                                               P_3k = G^_3k + s3 (s_k G^_k3 + s3 G^_3k) / d_k
 *     with FORCE_110:  P = 0 except P_12 = -P_21 = (G^_12 - G^_21) / (s1 + s2), P_k3 = (s_k G^_k3 + s3 G^_3k) / d_k,
 *                      P_3k = (s3 G^_k3 + s_k G^_3k) / d_k.  Nothing divides by s1 - s2: the gradient is finite at an exact
 *                      essential matrix (s1 = s2), where torch's svd_backward is singular.
 *   u = sum_{k != 9} q_k (q_k^T vec(g_F0)) / (lam_9 - lam_k);  r_i = A_i . f, g_A_i = r_i u + (A_i . u) f, g_w_i = a_i . g_A_i,
 *   g_a_i = w_i g_A_i, to p~ by the product rule, and g_p = scale / (1 + 1e-10) g_p~.
 *   With N = 8 the eight rows have an exact null vector: A f = 0 whatever the points and weights are, so r_i is taken as the
 *   constant 0 it is (not the rounding noise A_i . f evaluates to) and g_w is written as 0.
 * Guard rule: every denominator above (lam_9 - lam_k, s_k^2 - s3^2, s1 + s2), and the s1, s2 that normalise u1, u2, keeps its sign and has its magnitude floored at 1e-30
 * (guard_den16 of the fit adjoint): a repeated eigen- or singular value gives a large finite gradient, not a NaN.
 *
 * Launch shape: one wavefront per problem, four problems per workgroup; with S > 1 and point gradients asked for, a second launch
 * adds the sets' partial gradients [S,B,N,4] (fp64, in the workspace) in ascending set order.
 *
 * Refusals, made on the host before any HIP call, in this order: B < 0, N < 8 or n_weight_sets < 1: INVALID_ARG.  `flags` without
 * SQRT2 | NO_ROWNORM, or with a bit other than those two, FORCE_110 and NO_HARTLEY: INVALID_ARG.  Then B == 0 returns OK: nothing
 * is launched and nothing written.  A NULL X, Y, F_out or g_F, or g_X, g_Y and g_w all NULL: INVALID_ARG.  X, Y, g_X or g_Y not
 * 8-byte aligned: INVALID_ARG.  S > 1 with g_X or g_Y asked for and a NULL workspace or one not 16-byte aligned: INVALID_ARG.
 * S * B * N > 2^31 - 1: UNSUPPORTED.
 */
size_t dfepe_eight_point_bwd_workspace_bytes(int B, int N, int n_weight_sets);
int dfepe_eight_point_bwd(void *stream, const float *X, const float *Y, const float *w, int B, int N, int n_weight_sets,
                          unsigned flags, const float *F_out, const float *g_F,
                          float *g_X, float *g_Y, float *g_w, void *workspace);

/*
 * Adjoint of the DSAC loop: the gradients of dfepe_dsac's E_sample, score, E_refit, loss, quality and exp_loss w.r.t. the pixel
 * points X and Y (csrc/dsac_adjoint.hip, csrc/dsac_adjoint_math.h).  The conventions are dfepe_dsac's: fp32 in and out, fp64
 * inside, every output rounded once; no atomics, no allocation, no host synchronisation; one linear chain of eight launches (seven with H = 1, where the refits' adjoint needs no set sum) whatever
 * B and H are (capturable); a pair's bits do not depend on the run or on the rest of the batch; a non-finite input stays in its own
 * pair.  dfepe_version() stays 154 with this addition: nothing that existed changes.
 *
 * The function differentiated is the forward as dfepe_dsac documents it, stages 1-5 on the fp32 values it wrote; each fp32 rounding
 * between stages is taken as the identity.  K is a CONSTANT: its gradient is not built.  soft, sampson, counts, best and top_loss
 * take no upstream.  The Hartley transforms of both fits are constants, as in dfepe_eight_point_bwd.
 *
 *   X, Y, K, idx, B, N, H, S, inlier_beta, inlier_alpha, loss_kind: as given to dfepe_dsac (inlier_thresh is not read: `soft` is)
 *   E_sample [B,H,9], soft [B,H,N], score [B,H], E_refit [B,H,9], loss [B,H], counts [B,N]: the forward's outputs as written
 *   g_E_sample [B,H,9], g_score [B,H], g_E_refit [B,H,9], g_loss [B,H], g_quality [B,N], g_exp_loss [B]: upstream gradients, each
 *     may be NULL (= 0), not all of them
 *   g_X, g_Y [B,N,2] (8-byte aligned): written, not accumulated; one of the two may be NULL
 *   t_score, t_loss [B,H], t_E_refit [B,H,9], t_w [H,B,N], t_E_sample [B,H,9]: the stage totals below, each may be NULL (it then
 *     lives in the workspace only)
 *   workspace: dfepe_dsac_bwd_workspace_bytes(B, N, H, S) bytes, 16-byte aligned, contents irrelevant.  In floats, every section
 *     rounded up to a multiple of 4: 2 x 2BN (K^-1 points), 2 x 2BHS (gathered samples), BHN (weights), 2 x 9BH (E_refit and t_E_refit
 *     as [H,B,9]), BH, BH, 9BH, BHN, 9BH (the five totals), 2 x 2BN, 2 x 2BHS (the fits' point gradients), 2 x 18BH (F_h, M_h in fp64),
 *     and dfepe_eight_point_bwd_workspace_bytes(B, N, H) / 4.
 *
 * Launches, with p = softmax(alpha score) and Lbar = sum_h p_h loss_h recomputed in fp64 from the fp32 score and loss,
 * max-subtracted as the vote does:
 *   1 prep     the K^-1 points and the gathered samples (ds::inv3, ds::normalized_point) in the 2-D layout dfepe_eight_point_bwd reads;
 *              w = sqrt(soft) rounded to fp32 as the forward formed it, [H,B,N]; F_h = K^-T E_sample K^-1 and M_h (E_refit with
 *              loss_kind 1, K^-T E_refit K^-1 with 2) in fp64.  The forward's workspace is not kept: all of it is recomputed.
 *   2 head     t_loss = g_loss + g_exp_loss[b] p_h;  t_score = g_score + g_exp_loss[b] alpha p_h (loss_h - Lbar)
 *              + sum_{j<S} g_quality[b, idx[b,h,j]] / (counts[b, idx[b,h,j]] + 1e-10), in slot order; an index outside 0..N-1
 *              contributes nothing, as in the vote.
 *   3 loss     t_M = (t_loss / N) sum_n d sampson(M_h; x_n, y_n) / dM, summed in the order of the forward's stage 4;
 *              t_E_refit = g_E_refit + t_M (kind 1) or + K^-1 t_M K^-T (kind 2); = g_E_refit with loss_kind 0.
 *   4-5 refit  dfepe_eight_point_bwd with H weight sets, w, F_out = E_refit, g_F = t_E_refit, SQRT2 | NO_ROWNORM | FORCE_110:
 *              t_w [H,B,N] and the gradient to the K^-1 points summed over the sets.
 *   6 score    c[b,h,n] = -beta (1 - s)(s t_score + w t_w / 2), s the fp32 soft as written.  No division: where s = 0 (the
 *              reference's sqrt(1 - sigmoid) backpropagates inf * 0 = NaN there) c = 0, the limit of d sqrt(s)/dd =
 *              -(beta/2) sqrt(s)(1 - s); a NaN stays a NaN.  t_F = sum_n c d sampson(F_h)/dF, t_E_sample = g_E_sample + K^-1 t_F K^-T.
 *   7 sample   dfepe_eight_point_bwd on the B H gathered problems of S points, F_out = E_sample, g_F = t_E_sample.
 *   8 points   one lane per correspondence: the refit's K^-1 gradient plus the sample fits' of every (h, j) with idx[b,h,j] == n,
 *              through the Jacobian of _de_homo(K^-1 .) with its 1e-10 guard, plus the direct pixel terms
 *              sum_h [c d d_h/dx + (t_loss_h / N) d l_h/dx].  A workgroup owns 64 correspondences; its wavefront v adds the
 *              hypotheses [v Hq, (v+1) Hq), Hq = ceil(H/4), ascending, per hypothesis the slots ascending, then the score's term,
 *              then the loss's; wavefront 0 adds the four partial sums in wavefront order, the refit's gradient first.
 *
 * Refusals, made on the host before any HIP call, in this order: B or N < 0, H < 1, S outside 8..16, N < S, loss_kind outside 0..2:
 * INVALID_ARG.  Then B == 0 returns OK: nothing is launched and nothing written.  A NULL X, Y, K, idx, E_sample, soft, score,
 * E_refit, loss, counts or workspace: INVALID_ARG.  Every upstream NULL: INVALID_ARG.  g_X and g_Y both NULL: INVALID_ARG.  X, Y,
 * g_X or g_Y not 8-byte aligned, or a workspace that is not 16-byte aligned: INVALID_ARG.  B * H * N > 2^31 - 1: UNSUPPORTED.
 * Not built: the gradient to K, upstreams for soft, sampson and top_loss.
 */
size_t dfepe_dsac_bwd_workspace_bytes(int B, int N, int H, int S);
int dfepe_dsac_bwd(void *stream, const float *X, const float *Y, const float *K, const int *idx, int B, int N, int H, int S,
                   float inlier_thresh, float inlier_beta, float inlier_alpha, int loss_kind,
                   const float *E_sample, const float *soft, const float *score, const float *E_refit, const float *loss,
                   const float *counts,
                   const float *g_E_sample, const float *g_score, const float *g_E_refit, const float *g_loss, const float *g_quality,
                   const float *g_exp_loss,
                   float *g_X, float *g_Y,
                   float *t_score, float *t_loss, float *t_E_refit, float *t_w, float *t_E_sample,
                   void *workspace);

/*
 * The device-side sampler of the DSAC loop: idx [B,H,S] of dfepe_dsac drawn on the stream (csrc/sampler.hip, csrc/sampler_math.h),
 * uniformly (the law of random.sample(range(n), S) for the SET, dsac.py:46) or in proportion to per-correspondence weights without
 * replacement (np.random.choice(n, topK, p=p) of DeepFNetSampleLoss.Fit.forward).  Integer arithmetic only: the kernel, the host
 * build of sampler_math.h and the restatement tests/sampler_ref.py agree bit for bit.  No atomics, no allocation, no host
 * synchronisation, one linear chain of launches (two when weighted, else one): capturable, and with `counter` advanced by
 * dfepe_sampler_advance inside the capture every replay of the graph draws fresh sets.  dfepe_version() stays 154 with this addition:
 * nothing that existed changes.
 *
 *   seed, offset, counter   Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and counter = (k, h, b, off): block k of
 *        hypothesis h of pair b, off = offset + (counter ? *counter : 0) mod 2^32, `counter` one unsigned on the device, read by the
 *        kernel.  Block k gives the words 4k .. 4k+3; draw j of a hypothesis uses r64 = word[2j+1] << 32 | word[2j]: exactly 2 S words,
 *        no rejection loop.  A set depends on (seed, off, b, h, n, S) and its pair's weights only: not on B, H, the launch or the run.
 *   bounded integer   t = mulhi64(r64, range), bias at most range / 2^64 per draw (< 2^-33 uniform; weighted: range < N 2^30).
 *   n_valid [B] int32 or NULL (= N): only the first n = clamp(n_valid[b], S, N) correspondences of pair b can be drawn (the
 *        reference's matches_good_unique_nums).
 *   weights NULL: uniform mode, Floyd's subset algorithm: for i = 0 .. S-1, j = n - S + i, t = mulhi64(r64_i, j + 1), take j if t is
 *        already in the set, else t; indices in the order generated (the order within a set is not uniform and need not be: the fit and
 *        the vote are symmetric in the sample).  No memory is read but n_valid and counter; N up to 2^31 - 1.
 *   weights [B,N]: weighted mode.  Per pair: a weight that is NaN, +-inf or <= 0 has q = 0; m = the largest other weight among the
 *        first n, m = f 2^e with f in [0.5, 1); q_i = floor(w_i 2^(30 - e)) by shifting the significand (exact, no division), so
 *        max q lies in [2^29, 2^30) and weights below 2^-30 m have q = 0 and are never drawn.  Launch 1, one workgroup per pair,
 *        writes the exclusive prefix sums P[0 .. n] (uint64) in chunks of dfepe_sampler_scan_chunk() weights with a carry.  Draw k:
 *        total = P[n] - sum of the chosen q, t = mulhi64(r64_k, total); walk the chosen indices c in ascending order with rem = 0,
 *        while t + rem >= P[c] add q[c] to rem, stop at the first c where that fails; the index drawn is the largest i < n with
 *        P[i] <= t + rem (binary search): never a chosen one, never one with q = 0.
 *        A pair with fewer than S indices of q > 0 is drawn in uniform mode, and fallback[b] = 1.
 *   idx [B,H,S] int32: written; distinct within a hypothesis and in [0, n): dfepe_dsac's contract.
 *   fallback [B] int32 or NULL: 1 where a weighted pair was drawn uniformly, else 0 (always 0 in uniform mode).
 *   workspace: dfepe_sample_sets_workspace_bytes(B, N, weighted) bytes, 16-byte aligned, contents irrelevant: B (N + 2) uint64 (P and
 *        the number of q > 0 of every pair), rounded up to 16 bytes; 0 bytes (NULL allowed) when not weighted.
 * Launch 2: one lane per hypothesis, a grid tail draws nothing; each wavefront writes its sets as consecutive words.
 *
 * Refusals, made on the host before any HIP call, in this order: B or N < 0, H < 1, S outside 8..16, N < S: INVALID_ARG.  Then
 * B == 0 returns OK: nothing is launched and nothing written.  A NULL idx: INVALID_ARG.  Weighted with a NULL workspace or one that is
 * not 16-byte aligned: INVALID_ARG.  B * H * S > 2^31 - 1: UNSUPPORTED.  Weighted with N > 2^20: UNSUPPORTED.
 *
 * dfepe_sampler_advance: a one-thread launch, *counter += by (mod 2^32).  A NULL counter: INVALID_ARG.
 * Not built: a sampler that replays random.sample's Mersenne Twister stream.
 */
int dfepe_sampler_scan_chunk(void);
size_t dfepe_sample_sets_workspace_bytes(int B, int N, int weighted);
int dfepe_sample_sets(void *stream, int B, int N, int H, int S, unsigned long long seed, unsigned offset, const unsigned *counter,
                      const float *weights, const int *n_valid, int *idx, int *fallback, void *workspace);
int dfepe_sampler_advance(void *stream, unsigned *counter, unsigned by);

/*
 * The sample-loss branch (csrc/sample_loss.hip, csrc/sample_loss_math.h).
 * Replaces: Fit.forward of deepFEPE/models/DeepFNetSampleLoss.py:364-436 around its fits (np.random.choice(n, topK, p=p) 100 times per
 *           pair, torch.topk of get_unique, the three torch.gather, prod(1000 w) / (sum + 1e-10)) and loss_selected_F of
 *           deepFEPE/train_good_utils.py:387-426.  The fits themselves are dfepe_w8pt_fwd_shared / dfepe_w8pt_bwd on B H problems of K.
 * Notation: B pairs, N correspondences, H sets per pair (selects_each_sample = 100), K draws per set (topK = 20), M virtual points.
 * No kernel uses atomics, allocates or synchronises with the host; every sum has a fixed order (two runs agree bit for bit); each
 * entry is one launch (two for a weighted draw) on `stream`: a linear chain, capturable.  Floats are computed in fp64 and rounded
 * once.  dfepe_version() stays 154 with this addition: nothing that existed changes.
 *
 * dfepe_sample_multisets: idx [B,H,K] int32 drawn WITH replacement in proportion to weights [B,N] over the first
 *   n = clamp(n_valid[b], K, N) correspondences.  seed, offset, counter, the streams, n_valid, the quantisation q, the prefix sums
 *   P[0 .. n] and the workspace (dfepe_sample_sets_workspace_bytes(B, N, 1) bytes, 16-byte aligned) are those of dfepe_sample_sets
 *   with K in the place of S.  Draw j of set h of pair b: t = mulhi64(r64_j, P[n]); the index is the largest i < n with P[i] <= t
 *   (binary search).  One lane per set, exactly 2 K words (K odd: the last block's upper half is not used), no rejection loop.  A
 *   weight that is NaN, +-inf, <= 0 or below 2^-30 of the pair's largest (q = 0) is never drawn.  The bias of a draw is at most
 *   P[n] / 2^64 < N 2^-34.  A pair without any q > 0 is drawn uniformly with replacement, index = mulhi64(r64_j, n), and
 *   fallback[b] = 1 (fallback [B] int32 or NULL).  weights NULL: every pair is drawn that way, no workspace, fallback = 0.
 *   A set depends on (seed, off, b, h, n, K) and its pair's weights only.  dfepe_sampler_advance serves the counter.
 *   Refusals, on the host before any HIP call, in this order: B or N < 0, H < 1, K outside 8..32, N < K: INVALID_ARG.  B == 0
 *   returns OK.  A NULL idx: INVALID_ARG.  Weights with a NULL or misaligned workspace: INVALID_ARG.  B H K > 2^31 - 1:
 *   UNSUPPORTED.  Weights with N > 2^20: UNSUPPORTED.
 *
 * dfepe_topk_select: idx [B,K] int32 and, unless NULL, values [B,K]: the K largest of x[b, :n], n = clamp(n_valid[b], K, N) (n_valid
 *   NULL = N), in descending order.  The rule: values compare as floats (a denormal is its value, -0 = +0); equal values go lowest
 *   index first; NaN is greater than everything, as torch.topk orders it, lowest index first among NaNs.  One wavefront per pair,
 *   K rounds over the n values.
 *   Refusals in order: B < 0, N < 1, K < 1, K > N: INVALID_ARG.  B == 0: OK.  A NULL x or idx: INVALID_ARG.  B K > 2^31 - 1: UNSUPPORTED.
 *
 * dfepe_sample_gather: pts1, pts2 [B,N,3], weights [B,N], idx [B,H,K] -> pts1_sel, pts2_sel [B H,K,3], w_sel [B H,K] (exact copies, the
 *   layout the fit entry takes) and, unless NULL, accu [B,H] = prod_k (1000 w[idx_k]) / (sum over the pair's H products + 1e-10)
 *   (DeepFNetSampleLoss.py:418-419).  Product and sum are fp64, the quotient is rounded once.  This differs from the reference's
 *   float32 where its product overflows or underflows (float32 gives inf / NaN or 0 / 0-sum there; fp64 keeps 20 factors of 1e-12).
 *   An index outside [0, N) is the caller's error; it is clamped into range, never dereferenced.
 *   Refusals in order: B < 0, N, H or K < 1: INVALID_ARG.  B == 0: OK.  A NULL pointer other than accu: INVALID_ARG.
 *   B H K > 2^31 - 1: UNSUPPORTED.
 *
 * dfepe_sample_floss_fwd / _bwd: F_sel [B,H,9], T1, T2 [B,9] (t_stride = 9) or one [9] (t_stride = 0), virt1, virt2 [B,M,3].
 *   loss_sum [B,H] = sum over the M virtual points of compute_epi_residual(T1 virt1, T2 virt2, F_sel[b,h], clamp_at)
 *   (utils_F.py:400-413); T v is formed in fp64 and rounded to float as dfepe_floss_fwd does, the residual and its sum are fp64.
 *   Backward: g_loss_sum [B,H] -> g_F [B,H,9] (written); the gradient passes where the residual <= clamp_at.  One workgroup per pair:
 *   the pair's virtual points are read and transformed once, into LDS; one wavefront per set.  (dfepe_floss_fwd takes 16 layers.)
 *   Refusals in order: B < 0, H < 1, M < 1, t_stride not 0 or 9: INVALID_ARG.  B == 0: OK.  A NULL pointer: INVALID_ARG.
 *   M > dfepe_sample_loss_max_virt() (2048: 24 bytes of LDS per point) or B H > 2^31 - 1: UNSUPPORTED.
 *
 * dfepe_sample_scatter_bwd: g_w [B,N] (written) = for every correspondence the sum over the cells (h, k) of its pair that name it of
 *   g_w_sel[b,h,k] (NULL = 0) and, when g_accu [B,H] is given, of the adjoint of accu: accu[b,h] (g_accu[b,h] - G) / w, G = sum_h
 *   g_accu accu.  Repeats within a set and across sets all count; a correspondence never drawn gets exact 0.  One lane per
 *   correspondence walks the H K cells in order and sums in fp64; the cells are staged in LDS dfepe_sample_scatter_chunk() at a
 *   time, so H K has no limit.  Where w = 0 exactly the accu term is taken as 0 (torch differentiates the product through the other
 *   factors there; a weighted draw never returns such a correspondence).
 *   Refusals in order: B < 0, N, H or K < 1: INVALID_ARG.  B == 0: OK.  A NULL idx or g_w: INVALID_ARG.  g_accu with a NULL weights or
 *   accu: INVALID_ARG.  B H K > 2^31 - 1 or B > 65535: UNSUPPORTED.
 */
int dfepe_sample_loss_max_virt(void);
int dfepe_sample_scatter_chunk(void);
int dfepe_sample_multisets(void *stream, int B, int N, int H, int K, unsigned long long seed, unsigned offset, const unsigned *counter,
                           const float *weights, const int *n_valid, int *idx, int *fallback, void *workspace);
int dfepe_topk_select(void *stream, const float *x, const int *n_valid, int B, int N, int K, int *idx, float *values);
int dfepe_sample_gather(void *stream, const float *pts1, const float *pts2, const float *weights, const int *idx, int B, int N, int H,
                        int K, float *pts1_sel, float *pts2_sel, float *w_sel, float *accu);
int dfepe_sample_floss_fwd(void *stream, const float *F_sel, int B, int H, const float *T1, const float *T2, int t_stride,
                           const float *virt1, const float *virt2, int M, float clamp_at, float *loss_sum);
int dfepe_sample_floss_bwd(void *stream, const float *F_sel, int B, int H, const float *T1, const float *T2, int t_stride,
                           const float *virt1, const float *virt2, int M, float clamp_at, const float *g_loss_sum, float *g_F);
int dfepe_sample_scatter_bwd(void *stream, const float *g_w_sel, const float *g_accu, const float *weights, const float *accu,
                             const int *idx, int B, int N, int H, int K, float *g_w);

#ifdef __cplusplus
}
#endif
#endif /* DFEPE_H */
