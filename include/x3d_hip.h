/* x3d_hip.h -- C ABI of libx3d_hip.so: the MI355X (gfx950) X3D forward/backward hot path.
 *
 * The reference (fcogidi/X3D-tf) has no native/FFI layer: its boundary is the Python class
 * model.X3D plus the tf.keras layers it calls.  Every entry point below replaces one
 * group of tf.keras ops on that path; the citation after each declaration is the reference call
 * site it stands in for.  A reference maintainer binds these with ctypes.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every pointer is DEVICE memory unless marked host.
 *  - Activations are NCTHW, contiguous, element type `dtype` (X3D_F32, X3D_BF16 or X3D_F16).  Arithmetic,
 *    weights, per-channel coefficients and reductions are fp32 (statistics accumulate in fp64); with a 16-bit
 *    `dtype` the pointwise GEMM operands are rounded to that type for the matrix cores (fp32 accumulation).
 *  - `stream` is a hipStream_t passed as void*; all work is stream-ordered, nothing allocates,
 *    nothing synchronises; functions are re-entrant.
 *  - Return value: X3D_OK, or an error code with a message in x3d_last_error() (thread local).
 *  - Accumulating outputs (stats, sums, dw, pool) are += : the caller zeroes them (one memset of
 *    its workspace per step).
 */
#ifndef X3D_HIP_H
#define X3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define X3D_OK 0
#define X3D_ERR_INVALID 1
#define X3D_ERR_LAUNCH 2

#define X3D_F32 0
#define X3D_BF16 1
#define X3D_F16 2   /* IEEE half: the reference's only reduced-precision mode (Keras mixed_float16, utils.py:176-192) */

#define X3D_ACT_NONE 0
#define X3D_ACT_RELU 1
#define X3D_ACT_SWISH 2
#define X3D_ACT_SIGMOID 3

/* epilogues of x3d_pw_dgrad */
#define X3D_EPI_STORE 0       /* dx = W^T dY */
#define X3D_EPI_ADD 1         /* dx = W^T dY + add                     (identity shortcut) */
#define X3D_EPI_ADD_STRIDED 2 /* dx = W^T dY + upsample_zero(add, 2)   (shortcut conv, stride 2) */
#define X3D_EPI_SWISH_BWD 3   /* dv = (W^T dY) * swish'(gate*bn_b(braw)); per-(n,c) sums */

/* Version of THIS header: bumped with every incompatible change of a signature or struct.  x3d_version() returns the value
 * the library was built with; a binding must refuse a library whose version differs from the header it was written against
 * (x3d_tf_amd/hip.py does): a stale libx3d_hip.so would otherwise take shifted arguments silently.
 * History (latest): 133 x3d_subsample2; 134 x3d_topk_metrics (device-side accuracy / top-k counters for Trainer.fit);
 *   135 x3d_jpeg_parse / x3d_jpeg_decode (JPEG frames decoded on the device);
 *   136 x3d_sigmoid_bce / x3d_view_max / x3d_multilabel_ap (multi-label head and mAP);
 *   137 x3d_mix_clips / x3d_mix_targets / x3d_softmax_xent_soft (mixup, CutMix and label smoothing);
 *   138 x3d_train_clips_aug (batched training augmentation: random-resized crop, colour jitter, random erasing);
 *   138 (additions only, no bump) x3d_drop_path_draw / x3d_tail_fwd_dp / x3d_tail_bwd_dp (stochastic depth);
 *   138 (additions only, no bump) x3d_seg_sumsq / x3d_lars / x3d_adamw / x3d_lamb (layer-wise optimizers);
 *   138 (additions only, no bump) x3d_precise_bn_accum / x3d_precise_bn_final (precise BatchNorm statistics);
 *   138 (additions only, no bump) x3d_seg_grad_sumsq / x3d_sgd_pt / x3d_adam_pt / x3d_lars_pt / x3d_adamw_pt / x3d_lamb_pt
 *       (fine-tuning: frozen tensors and per-tensor learning rates);
 *   138 (additions only, no bump) x3d_softmax_xent_kd / x3d_sigmoid_bce_kd (knowledge distillation);
 *   138 (additions only, no bump) x3d_loss_scale_apply / x3d_unscale_sumsq / x3d_seg_unscale_sumsq / x3d_loss_scale_update
 *       (the fp16 loss scaler on the device);
 *   138 (additions only, no bump) x3d_stem_kernel_name (dry-run dispatch of the six stem entry points);
 *   138 (additions only, no bump) frozen BatchNorm backward: a negative count in x3d_bn_bwd_finalize / _rc and
 *       x3d_se_bnb_bwd_args.P (values every earlier version refused; no struct changes its layout);
 *   138 (additions only, no bump) x3d_softmax_xent_w / x3d_sigmoid_bce_w / x3d_class_hits (class and sample weights,
 *       focal terms, per-class hit counters);
 *   138 (additions only, no bump) x3d_roi_pool_fwd / x3d_roi_pool_bwd (ROI head for action detection);
 *   138 (additions only, no bump) x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil / x3d_dw3d_kernel_name_dil (dilated channelwise convs of
 *       a stride-1 res5 for detection; no struct changes its layout);
 *   138 (additions only, no bump) x3d_frame_match / x3d_frame_ap (frame-mAP for action detection). */
#define X3D_ABI_VERSION 138
int x3d_version(void);
const char* x3d_last_error(void);

/* ------------------------------------------------------------------------------------------
 * K1  stem spatial conv: tf.pad(0,1,1) + Conv3D(k=(1,3,3), s=(1,2,2), valid, no bias)
 *     reference model.py:161-166,178-184,203-204
 *     x [N][Cin][T][H][W] -> y [N][Cout][T][Ho][Wo], Ho=(H-1)/2+1.  w [Cout][Cin][3][3] fp32.
 *     x_layout = X3D_LAYOUT_NTHWC (ABI 127): x is the caller's channels-last clip batch [N][T][H][W][Cin] itself -- the
 *     layout of the reference's input (model.py:113) -- read in place by the matrix-core kernels (16-bit storage, Cin = 3,
 *     W % 8 == 0, 16-byte aligned: x3d_stem_s_nthwc_supported); no x3d_nthwc_to_ncthw pass and no planar copy of the batch.
 * ------------------------------------------------------------------------------------------ */
#define X3D_LAYOUT_NCTHW 0
#define X3D_LAYOUT_NTHWC 1
int x3d_stem_s_nthwc_supported(int Cin, int W, int Cout, int dtype);
int x3d_stem_s_fwd(const void* x, const float* w, void* y, int N, int Cin, int T, int H, int W,
                   int Cout, int dtype, int x_layout, void* stream);
/* dW of the same conv (the input needs no gradient).  dy = grad wrt y.  dw [Cout][Cin][3][3] += */
int x3d_stem_s_wgrad(const void* x, const void* dy, float* dw, int N, int Cin, int T, int H, int W,
                     int Cout, int dtype, int x_layout, void* stream);

/* ------------------------------------------------------------------------------------------
 * K2  stem temporal depthwise conv: tf.pad(KT/2,0,0) + Conv3D(k=(KT,1,1), groups=C, no bias)
 *     reference model.py:170-175,187-194,205-206.   x,y [N][C][T][HW]; w [C][KT] fp32.
 *     stats [C][2] += (sum, sum of squares) of y as stored.
 *     INFERENCE epilogue (out_scale_shift [C][2] != NULL; stats must be NULL): y = out_act(s*conv + t) -- the stem's
 *     BatchNorm folded from the moving statistics + ReLU (model.py:196-200,207-208), so the raw conv output is not stored.
 * ------------------------------------------------------------------------------------------ */
int x3d_dwt_fwd(const void* x, const float* w, void* y, double* stats, const float* out_scale_shift, int out_act, int N,
                int C, int T, int HW, int KT, int dtype, void* stream);
/* backward of K2 through the stem's BN+ReLU: dY = A*g + B*yraw + C (coef [C][4]), g = grad wrt relu(bn(y)) masked by
 * the sign of bn(y).
 *   relu_scale_shift == NULL : g is already masked (x3d_relu_bn_bwd_reduce wrote it);
 *   relu_scale_shift [C][2]  : g is the UNMASKED gradient and the mask [s*yraw + t > 0] is applied here, on the yraw values
 *                              the kernel loads anyway -- x3d_relu_bn_bwd_reduce then runs with g == NULL (sums only) and
 *                              the masked gradient is never written or re-read (one tensor pass less each way).
 * dx [N][C][T][HW] = conv_t^T dY ; dw [C][KT] += */
int x3d_dwt_bwd(const void* g, const void* yraw, const float* relu_scale_shift, const float* coef, const void* x,
                const float* w, void* dx, float* dw, int N, int C, int T, int HW, int KT, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * K1 + K2 FUSED (ABI 131): the whole stem convolution pair, reference model.py:202-206 -- conv_s, then conv_t, with nothing
 *     in between -- as one launch each way, so neither the conv_s output nor its gradient ever exists in HBM.
 *   x3d_stem_fwd: x (channels-last clip batch [N][T][H][W][3], X3D_LAYOUT_NTHWC) -> y [N][Cout][T][Ho][Wo] = conv_t(conv_s(x)),
 *     the conv_s output rounded to the storage type between the two exactly as x3d_stem_s_fwd stores it: y is bit-identical to
 *     x3d_stem_s_fwd + x3d_dwt_fwd.  stats / out_scale_shift / out_act as in x3d_dwt_fwd.
 *   x3d_stem_bwd: g (grad wrt relu(bn(y)), masked here when relu_scale_shift != NULL), yraw (= y of the forward), coef as in
 *     x3d_dwt_bwd; dw_t [Cout][KT] += , dw_s [Cout][3][3][3] += .  The conv_s output is recomputed on the matrix cores, the
 *     conv_t input gradient stays in LDS as the operand of the conv_s weight-gradient tile.
 *   x3d_stem_fused_supported: bit 0 = x3d_stem_fwd takes the shape (16-bit storage, x_layout = X3D_LAYOUT_NTHWC, Cin = 3,
 *     W % 8 == 0, Cout <= 32, KT = 5, x and y under 2 GB; x 16-byte aligned), bit 1 = x3d_stem_bwd takes it and is the faster
 *     backward (Cout <= 24; it runs, slower than K2 + K1's backward, up to 32).  Everything else runs the separate K1 / K2 entry
 *     points above.
 * ------------------------------------------------------------------------------------------ */
int x3d_stem_fused_supported(int Cin, int Cout, int KT, int N, int T, int H, int W, int dtype, int x_layout);
int x3d_stem_fwd(const void* x, const float* w_s, const float* w_t, void* y, double* stats, const float* out_scale_shift,
                 int out_act, int N, int Cin, int T, int H, int W, int Cout, int KT, int dtype, int x_layout, void* stream);
int x3d_stem_bwd(const void* g, const void* yraw, const float* relu_scale_shift, const float* coef, const void* x,
                 const float* w_s, const float* w_t, float* dw_s, float* dw_t, int N, int Cin, int T, int H, int W, int Cout,
                 int KT, int dtype, int x_layout, void* stream);
/* Name of the kernel instantiation one of the six stem entry points above would launch, every template argument included
 * ("stem_s_fwd_bf16_kernel<f16,4,nhwc>", "dwt_bwd_kernel<bf16,2,7>"), without launching anything: the entry's own checks and path
 * decisions in dry-run mode (works without a GPU, makes no HIP call).  entry = the entry point's name ("x3d_dwt_bwd").
 * a .. d = the addresses of its tensor operands in its own argument order, inspected for alignment only:
 *   x3d_stem_s_fwd (x, y)   x3d_stem_s_wgrad (x, dy)   x3d_dwt_fwd (x, y)   x3d_dwt_bwd (g, yraw, x, dx)
 *   x3d_stem_fwd (x, y)     x3d_stem_bwd (g, yraw, x);  the rest NULL.
 * flags = the launch form, X3D_STEM_NAME_*: statistics given, out_scale_shift given, out_act = ReLU (forward entries),
 * relu_scale_shift given (backward entries).  Extents as the entry takes them; x3d_dwt_fwd / x3d_dwt_bwd read C = Cout and
 * HW = H * W (H, W: the plane conv_t runs on).  Returns what the entry would: an error where it refuses the launch. */
#define X3D_STEM_NAME_STATS 1
#define X3D_STEM_NAME_OUT_SS 2
#define X3D_STEM_NAME_OUT_RELU 4
#define X3D_STEM_NAME_RELU_SS 8
int x3d_stem_kernel_name(const char* entry, const void* a, const void* b, const void* c, const void* d, int flags, int N,
                         int Cin, int T, int H, int W, int Cout, int KT, int dtype, int x_layout, char* out, int cap);

/* ------------------------------------------------------------------------------------------
 * K3  BatchNormalization(axis=-1, eps, momentum)   reference model.py:89-92,196-199,254-257,
 *     268-271,300-303,368-371.
 *   finalize (training): stats [C][2] (sum, sumsq over `count` elements per channel) ->
 *     scale_shift [C][2] = (gamma*invstd, beta - mean*gamma*invstd), mean_invstd [C][2];
 *     if update_moving: moving = moving*momentum + batch*(1-momentum) (variance unbiased).
 *   eval_coef (inference): same outputs from the moving statistics.
 *   bwd_finalize: sums [C][2] = (sum g, sum g*yraw) -> coef [C][4] = (A,B,C,0) such that
 *     dYraw = A*g + B*yraw + C ; dgamma [C] += , dbeta [C] += .
 *   FROZEN statistics (SOLVER.FREEZE_BN: a trained layer normalised with its moving statistics): the forward pass takes
 *     scale_shift / mean_invstd from eval_coef and runs no finalize; backward, mean and invstd are constants, so
 *     dYraw = gamma*invstd*g.  A caller asks for that form with a NEGATIVE count -- the one rule of the launches that finalize a
 *     BatchNorm's backward pass: `count` of x3d_bn_bwd_finalize / x3d_bn_bwd_finalize_rc, and P of x3d_se_bnb_bwd_args (whose
 *     |P| is still the points per sample).  Then A = gamma*invstd, B = C = +0 exactly (a branch, not arithmetic on a large
 *     count), and dgamma / dbeta are the same expressions -- the same bits -- as in the batch form: invstd*(sum g*yraw -
 *     mean*sum g) and sum g with the moving mean / invstd in mean_invstd.  count = 0 stays an error.  x3d_bn_bwd_fold (the
 *     finalize derived by a consumer) has NO frozen form and still refuses count <= 0: give a frozen layer the launch.
 * ------------------------------------------------------------------------------------------ */
int x3d_bn_finalize(const double* stats, double count, const float* gamma, const float* beta,
                    float* moving_mean, float* moving_var, float eps, float momentum,
                    int update_moving, float* scale_shift, float* mean_invstd, int C, void* stream);
/* REPLICATED STATISTICS.  Every `stats` accumulator of this ABI (x3d_pw_fwd, x3d_dw3d_fwd, x3d_dwt_fwd producers;
 * x3d_bn_finalize, x3d_bn_fold consumers) is x3d_stats_replicas() copies of [C][2] doubles, x3d_stats_stride(C) doubles
 * apart: a producer workgroup adds into the copy its block index selects, the consumers sum the copies.  With ONE copy
 * every workgroup of a launch ends with fp64 atomics on the same C*2 addresses (one or two L2 channels): 10-18 us per
 * forward GEMM of X3D-M measured in isolation (216->96 @ 14x14: 68.8 -> 58.4 us; 108->48 @ 28x28: 92.8 -> 77.1 us), pointwise
 * forward 4.42 -> 4.08 ms per train step.  Buffers are zeroed by the caller: x3d_stats_replicas() * x3d_stats_stride(C)
 * doubles. */
int x3d_stats_replicas(void);
long long x3d_stats_stride(int C);

/* finalize FOLDED INTO THE CONSUMER (training): the consumer of a BatchNorm whose channel is uniform per workgroup
 * (x3d_dw3d_fwd for bn_a, x3d_tail_fwd_bn for bn_c / bn_r / the stem BN) computes scale/shift from the raw statistics
 * itself -- the same arithmetic as x3d_bn_finalize, bit for bit -- and one designated workgroup per channel writes
 * scale_shift / mean_invstd (kept for the backward pass) and updates the moving statistics.  Saves one ~6 us launch
 * between producer and consumer per layer (57 per X3D-M train step). */
typedef struct {
  const double* stats;         /* [C][2] (sum, sum of squares) of the producer's raw output */
  double count;                /* elements per channel */
  const float* gamma;
  const float* beta;
  float* moving_mean;          /* updated when update_moving */
  float* moving_var;
  float eps;
  float momentum;
  int update_moving;
  float* scale_shift;          /* out [C][2] */
  float* mean_invstd;          /* out [C][2] */
} x3d_bn_fold;
/* inference coefficients (scale, shift, mean, invstd from the moving statistics): all BatchNorm layers of a model in ONE launch (inference: 84-171 layers, else one ~5 us launch each per forward).
 * `items` is an array in DEVICE memory. */
typedef struct {
  const float* gamma; const float* beta; const float* moving_mean; const float* moving_var;
  float* scale_shift;          /* out [C][2] */
  float* mean_invstd;          /* out [C][2] */
  int C;
} x3d_bn_eval_item;
int x3d_bn_eval_coef_batched(const x3d_bn_eval_item* items, int n_items, float eps, void* stream);
int x3d_bn_bwd_finalize(const double* sums, double count, const float* mean_invstd,
                        const float* gamma, float* coef, float* dgamma, float* dbeta, int C,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * K3p precise BatchNorm (NETWORK.BN.USE_PRECISE_STATS; PySlowFast BN.USE_PRECISE_STATS / NUM_BATCHES_PRECISE, fvcore
 *     update_bn_stats): the moving statistics recomputed exactly from K training-mode forward passes instead of trusted to
 *     the momentum blend.  Added under ABI 138 without a version bump: new symbols and constants only.
 *     The raw fp64 sums are already on the device: every training plan keeps, per BatchNorm layer, the replicated `stats`
 *     accumulator its producer added into (REPLICATED STATISTICS above), intact after a forward pass.  So pooling K batches is
 *     one small launch per batch and one at the end; no second pass over activations, nothing returns to the host.
 *   table  [nlayers][X3D_PBN_COLS] int64 in DEVICE memory, one row per BatchNorm layer:
 *            X3D_PBN_STATS   address of the layer's `stats` accumulator (x3d_stats_replicas() copies, x3d_stats_stride(C) apart)
 *            X3D_PBN_C       channels
 *            X3D_PBN_COUNT   elements per channel the producer summed in one forward pass (N*T*H*W of the layer's output)
 *            X3D_PBN_MEAN    element offset of the layer's moving mean [C] in `params`
 *            X3D_PBN_VAR     element offset of its moving variance [C] in `params`
 *            X3D_PBN_POOLED  element offset of its [C][2] (sum, sum of squares) in `pooled`
 *          The kernels trust the table: the caller builds and checks it (x3d_tf_amd/plan.py).  Tables of different batch
 *          shapes differ in X3D_PBN_STATS and X3D_PBN_COUNT only and may feed the same `pooled`.
 *   pooled one fp64 buffer, the caller's, zeroed before the first batch: nlayers pooled counts, then every layer's [C][2] sums
 *          at its X3D_PBN_POOLED offset (>= nlayers).  One buffer, so that ONE all-reduce (sum) pools data-parallel ranks.
 *   x3d_precise_bn_accum: per channel, the copies of `stats` are added in the pairwise tree of x3d_bn_finalize / x3d_bn_fold
 *          (eights as ((0+1)+(2+3))+((4+5)+(6+7)), then (q0+q1)+(q2+q3)) and the totals added to `pooled`; one thread per
 *          layer adds X3D_PBN_COUNT to the layer's count slot.  One thread per channel, no atomics, a fixed order: the same
 *          inputs give the same bits on every run.  `stats` is read only.
 *   x3d_precise_bn_final: with n = the pooled count, per channel  mean = S1 / n ; var = max(S2 / n - mean^2, 0) ;
 *          unb = n > 1 ? var * (n / (n - 1)) : var ;  params[X3D_PBN_MEAN + c] = (float)mean, params[X3D_PBN_VAR + c] =
 *          (float)unb -- what x3d_bn_finalize hands to its moving update: after ONE accum the result equals, bit for bit, what
 *          x3d_bn_finalize(momentum = 0, update_moving = 1) writes from the same accumulator.  Whatever the moving statistics
 *          held is overwritten.  A layer whose pooled count is 0 gets NaN: run at least one accum first.
 *   One launch each, all layers at once.  Refused before the launch (X3D_ERR_INVALID): a null pointer, nlayers < 1, a table
 *   or pooled pointer that is not 8-byte, a params pointer that is not 4-byte aligned.
 * ------------------------------------------------------------------------------------------ */
#define X3D_PBN_COLS 6
#define X3D_PBN_STATS 0
#define X3D_PBN_C 1
#define X3D_PBN_COUNT 2
#define X3D_PBN_MEAN 3
#define X3D_PBN_VAR 4
#define X3D_PBN_POOLED 5
int x3d_precise_bn_accum(const long long* table, int nlayers, double* pooled, void* stream);
int x3d_precise_bn_final(const long long* table, int nlayers, const double* pooled, float* params, void* stream);

/* ------------------------------------------------------------------------------------------
 * K5  pointwise Conv3D(k=1, no bias) as a GEMM over points on MFMA: bottleneck a / c, shortcut
 *     `residual` (stride (1,s,s) valid), conv5.  reference model.py:246-253,292-299,360-367,80-87
 *     Input prologue (folded producer BN / SE gate / activation), applied on load:
 *       v = x ; if in_scale_shift: v = s*v + t ; if in_gate: v *= gate[n][ci] ; v = act(v)
 *     Epilogue: y stored raw; stats [Cout][2] += (sum, sumsq) of y as stored (may be NULL).
 *     INFERENCE epilogue (out_scale_shift != NULL; stats must be NULL): the BatchNorm that follows the conv -- folded from
 *     the moving statistics, model.py:300-303,368-371 -- and the residual Add + ReLU (model.py:381-392) run on the fp32
 *     accumulators, so neither the raw conv output nor a separate tail pass touches HBM:
 *       v = s_o*acc + t_o ; if out_add: v += (out_add_scale_shift ? s_r*add + t_r : add) ; y = out_act(v)
 *     (`c` conv of a block: out_add = block input (identity) or the raw shortcut conv output with bn_r as
 *     out_add_scale_shift; out_act = ReLU).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* x;               /* [N][Cin][T][H][W] */
  const float* w;              /* [Cout][Cin] fp32 */
  void* y;                     /* [N][Cout][T][Ho][Wo], Ho = ceil(H/stride) */
  double* stats;               /* [Cout][2] or NULL */
  const float* in_scale_shift; /* [Cin][2] or NULL */
  const float* in_gate;        /* [N][Cin] or NULL */
  int in_act;
  int N, Cin, Cout, T, H, W, stride, dtype;
  const void* w_panel;         /* optional (bf16 path): forward panel from x3d_pw_pack_weights, else NULL */
  /* folded residual tail (training; NULL: off).  x is then the raw `c` output of the block BELOW and the conv input is that
   * block's output, built on load and stored for its other readers -- the work of a separate x3d_tail_fwd pass:
   *   v = relu(s*x + t + (in_add_scale_shift ? s_r*in_add + t_r : in_add)) ;  in_store = v
   * (s, t) = in_scale_shift, in_act = X3D_ACT_RELU, no in_gate; 16-bit storage, stride 1: x3d_pw_fwd_tail_supported().
   * in_store without in_add: v = relu(s*x + t) -- the stem's BatchNorm + ReLU (x = the raw conv_t output, reference
   * model.py:202-210) folded into the first block's `a` conv. */
  const void* in_add;               /* [N][Cin][P]: raw shortcut-conv output of the block below, or its input (identity); NULL: no Add */
  const float* in_add_scale_shift;  /* [Cin][2] (bn_r of the block below) or NULL */
  void* in_store;                   /* [N][Cin][P] the block's output y */
  const float* out_scale_shift;     /* [Cout][2] or NULL (training form: raw store + stats) */
  const void* out_add;              /* [N][Cout][T][Ho][Wo] or NULL */
  const float* out_add_scale_shift; /* [Cout][2] applied to out_add, or NULL */
  int out_act;                      /* X3D_ACT_NONE / X3D_ACT_RELU */
} x3d_pw_fwd_args;
int x3d_pw_fwd(const x3d_pw_fwd_args* a, void* stream);
int x3d_pw_fwd_tail_supported(const x3d_pw_fwd_args* a);   /* 1: the in_add / in_store form covers this call */

/* BatchNorm-backward finalize folded into its consumers (coef_fold of the three backward argument structs below; NULL: off).
 * The coefficient table `coef` [C][4] of dYraw = A*g + B*yraw + C is x3d_bn_bwd_finalize's output: a ~6 us launch between
 * the kernel that produced the sums and the kernel that needs the table.  With coef_fold set the consuming kernel derives the
 * coefficients it needs from the sums itself, in its coefficient-table prologue (the same arithmetic, one definition:
 * the same bits), and `coef` is not read.  dgamma / dbeta non-NULL: workgroup (0, 0, 0) of the launch also adds the channel's
 * gamma / beta gradient (+=) and writes the table to coef_out -- exactly ONE launch per BatchNorm and step must be given them
 * (a data- and a weight-gradient launch that share a BatchNorm: one of the two).  x3d_pw_coef_fold_supported(): whether the
 * kernel behind a call takes it (the persistent weights-stationary kernels and the 16-bit weight-gradient kernel; the
 * entry points refuse the field otherwise). */
typedef struct {
  const double* sums;          /* [C][2] as x3d_bn_bwd_finalize takes them */
  double count;                /* > 0 (no frozen form here: K3) */
  const float* mean_invstd;    /* [C][2] */
  const float* gamma;          /* [C] */
  float* dgamma;               /* [C] += , or NULL */
  float* dbeta;                /* [C] += , or NULL */
  float* coef_out;             /* [C][4], or NULL (written with dgamma / dbeta) */
} x3d_bn_bwd_fold;

/* data gradient: dYraw = A*g + B*yraw + C on load (coef [Cout][4]; NULL coef: dYraw = g),
 * dx = W^T dYraw with one of the X3D_EPI_* epilogues. All tensors at the conv's OUTPUT points. */
typedef struct {
  const void* g;               /* [N][Cout][P] grad wrt the BN output of this conv */
  const void* yraw;            /* [N][Cout][P] raw conv output (NULL iff coef NULL) */
  const float* coef;           /* [Cout][4] or NULL */
  const float* w;              /* [Cout][Cin] fp32 */
  void* dx;                    /* [N][Cin][P] */
  int epi;
  const void* add;             /* EPI_ADD: [N][Cin][P];  EPI_ADD_STRIDED: [N][Cin][T][ceil(H/2)][ceil(W/2)] */
  const void* braw;            /* EPI_SWISH_BWD: [N][Cin][P] raw depthwise output */
  const float* b_scale_shift;  /* EPI_SWISH_BWD: [Cin][2] */
  const float* gate;           /* EPI_SWISH_BWD: [N][Cin] or NULL */
  double* nc_sums;             /* EPI_SWISH_BWD: [N][Cin][2] += (sum dv, sum dv*braw) */
  int N, Cin, Cout, T, H, W, dtype; /* T,H,W: extents of the P = T*H*W output points */
  const void* w_panel;         /* optional (bf16 path): dgrad panel from x3d_pw_pack_weights, else NULL */
  const x3d_bn_bwd_fold* coef_fold; /* NULL | derive `coef` from the BatchNorm-backward sums (above) */
} x3d_pw_dgrad_args;
int x3d_pw_dgrad(const x3d_pw_dgrad_args* a, void* stream);

/* fused data + weight gradient of one pointwise conv (bf16 storage, <= 128 channels on either side, stride 1):
 * ONE pass over g / yraw instead of the two that x3d_pw_dgrad + x3d_pw_wgrad make, and for the `c` conv one
 * pass over braw (swish for dw and swish' for dx from the same load).  Fields as in the two structs above:
 *   epi = X3D_EPI_ADD / X3D_EPI_ADD_STRIDED : `a` conv; x = conv input [N][Cin][P], add as in dgrad
 *   epi = X3D_EPI_SWISH_BWD                 : `c` conv; the conv input is swish(gate * (s_b*braw + t_b)); x unused
 * w_panel is the DGRAD panel of x3d_pw_pack_weights (required).  x3d_pw_bwd_supported() says whether a launch
 * is covered (shape, alignment); x3d_pw_bwd fails with X3D_ERR_INVALID otherwise -- callers then use the pair. */
typedef struct {
  const void* g;               /* [N][Cout][P] */
  const void* yraw;            /* [N][Cout][P] */
  const float* coef;           /* [Cout][4] */
  const void* w_panel;         /* dgrad panel (bf16) */
  void* dx;                    /* [N][Cin][P] */
  int epi;
  const void* add;
  const void* braw;
  const float* b_scale_shift;
  const float* gate;
  double* nc_sums;
  const void* x;               /* [N][Cin][P] conv input (ADD epilogues) */
  float* dw;                   /* [Cout][Cin] += */
  int N, Cin, Cout, T, H, W, dtype;
  /* folded residual-tail backward (ADD epilogues; tail_c == NULL: off).  The conv input x is the OUTPUT y of the previous
   * residual block, so dx is the gradient that block's Add + ReLU receives (model.py:381-392): with tail_c set the
   * epilogue applies that backward instead of a separate x3d_tail_bwd pass over dx,
   *   dx = [x > 0] * (W^T dYraw + add) ;  tail_sums_c [Cin][2] += (sum dx, sum dx*tail_c) ;
   *   tail_r != NULL (the previous block has a shortcut conv): tail_sums_r [Cin][2] += (sum dx, sum dx*tail_r)
   * tail_c / tail_r: raw c-conv / shortcut-conv outputs of the previous block, [N][Cin][P]. */
  const void* tail_c;
  const void* tail_r;
  double* tail_sums_c;
  double* tail_sums_r;
  /* RECOMPUTED conv output (ADD epilogues; rc_panel == NULL: off).  The conv is followed by a training-mode BatchNorm, so
   * dYraw = A*g + B*yraw + C with yraw = W x linear in the conv input: with rc_panel set the launch streams g and x ONLY
   * (yraw / coef / dw / w_panel are not read and may be NULL) -- the caller need not keep the conv's raw output at all:
   *   dx = [W1 | M] [g ; x] + c0 (+ add, + tail)    W1 = W^T diag(A), M = W^T diag(B) W, c0 = W^T C   (x3d_pw_bwd_rc_prepare)
   *   rc_sums [Cout + 1 + Cin][Cin] += [g ; 1 ; x] x^T  over all points (zero it before the launch); x3d_pw_bwd_rc_finish turns
   *   the sums into dw = diag(A) (g x^T) + diag(B) W (x x^T) + C (sum x)^T   (reference model.py:246-257 `a` -> `bn_a`). */
  const void* rc_panel;        /* x3d_pw_bwd_rc_panel_elems(Cout, Cin) elements of the storage type, 16-byte aligned */
  const float* rc_c0;          /* [Cin] */
  float* rc_sums;              /* x3d_pw_bwd_rc_sums_elems(Cout, Cin) floats */
  /* ... of a strided shortcut conv (reference model.py:360-367; rc_panel form only, epi = X3D_EPI_STORE: dx [N][Cin][T][H][W] is
   * the gradient at the SAMPLED pixels, the operand of the `a` backward's X3D_EPI_ADD_STRIDED): x_stride = 2, x is the block
   * input [N][Cin][T][xH][xW] with H = ceil(xH / 2), W = ceil(xW / 2).  x_stride = 0 / 1: dense (x [N][Cin][T][H][W]). */
  int x_stride, xH, xW;
  /* PARTIAL weight-gradient slabs instead of fp32 atomics (dw_slab == NULL: off, dw += by atomics).  The persistent
   * weights-stationary kernels (one workgroup per CU, each with its own [Cout][Cin] partial sum) end in a flush of
   * workgroups x Cout x Cin floats; as device-scope atomics that runs at ~1.3 TB/s whatever the schedule (measured: 13-24 us of
   * a 85-105 us launch), as plain stores into a slab per workgroup at the store rate.  With dw_slab the launch writes
   * x3d_pw_bwd_dw_parts(a) slabs of Cout * Cin floats (dw is not touched) and a LATER launch adds them up in a fixed order:
   * x3d_dw_slab_reduce, or the two reduce slots of x3d_se_bnb_bwd (a small launch that is on the critical path anyway).
   * x3d_pw_bwd_dw_parts() == 0: the kernel behind this call has no slab form (leave dw_slab NULL) -- also where Cout * Cin is
   * not a multiple of 4: the reduce adds the slabs up in aligned float4s. */
  float* dw_slab;              /* x3d_pw_bwd_dw_parts(a) * Cout * Cin floats, 16-byte aligned */
  int dw_slab_parts;           /* (ABI 132) the number of slabs dw_slab holds = what x3d_pw_bwd_dw_parts(a) returned when the buffer was
                                * sized: a launch whose grid differs (another device, another build switch between recording and
                                * replay) is refused instead of writing past the buffer or leaving slabs unwritten */
  const x3d_bn_bwd_fold* coef_fold; /* NULL | derive `coef` from the BatchNorm-backward sums (x3d_bn_bwd_fold) */
} x3d_pw_bwd_args;
int x3d_pw_bwd_supported(const x3d_pw_bwd_args* a);
int x3d_pw_bwd(const x3d_pw_bwd_args* a, void* stream);
int x3d_pw_bwd_dw_parts(const x3d_pw_bwd_args* a);
/* dw [elems] += sum over `parts` slabs of [elems] floats, parts in ascending order per element (deterministic) */
typedef struct {
  const float* slab;           /* NULL: no job */
  float* dw;
  int parts, elems;
} x3d_dw_reduce_job;
int x3d_dw_slab_reduce(const x3d_dw_reduce_job* jobs, int n_jobs, void* stream);
/* the per-step operands of the recomputed-output form.  panel_elems == 0: the layer shape is not covered (covered: Cin <= 32
 * with Cout <= 127; Cin 33..48 with Cout 65..127 or 193..223 -- the X3D stage-3 `a` convs and the first one of stage 4).  prepare: after x3d_bn_bwd_finalize produced `coef` [Cout][4]; finish: after x3d_pw_bwd, dw [Cout][Cin] +=. */
long long x3d_pw_bwd_rc_panel_elems(int Cout, int Cin);
long long x3d_pw_bwd_rc_sums_elems(int Cout, int Cin);
int x3d_pw_bwd_rc_prepare(const float* w /* [Cout][Cin] fp32 */, const float* coef, void* rc_panel, float* rc_c0, int Cout, int Cin,
                          int dtype, void* stream);
int x3d_pw_bwd_rc_finish(const float* rc_sums, const float* w, const float* coef, float* dw, int Cout, int Cin, int dtype, void* stream);
/* x3d_bn_bwd_finalize (arguments up to C: the same arithmetic, the same outputs) + x3d_pw_bwd_rc_prepare for the conv this
 * BatchNorm follows (w != NULL: its [C][Cin] weights; C <= 223) + x3d_pw_bwd_rc_finish of an EARLIER recomputed-output launch
 * (fin_sums != NULL), in ONE launch: three ~5 us launches of the backward pass's critical path become one. */
int x3d_bn_bwd_finalize_rc(const double* sums, double count, const float* mean_invstd, const float* gamma, float* coef,
                           float* dgamma, float* dbeta, int C, const float* w, void* rc_panel, float* rc_c0, int Cin,
                           const float* fin_sums, const float* fin_w, const float* fin_coef, float* fin_dw, int fin_Cout,
                           int fin_Cin, int dtype, void* stream);

/* bf16 weight panels.  The bf16 GEMMs keep their A operand (the weights) resident in LDS as bf16 rows of
 * pitch roundup(K,16)+8; without a panel every workgroup converts its rows from the fp32 master weights
 * (a latency-serialised gather that dominates small-P layers).  x3d_pw_pack_weights converts every
 * pointwise weight of the model once per step, in ONE launch, into the exact LDS image:
 *   fwd_panel   bf16 [roundup(Cout,32)][roundup(Cin,16)+8]   row co, column ci   (zero padded)
 *   dgrad_panel bf16 [roundup(Cin,32)][roundup(Cout,16)+8]   row ci, column co   (may be NULL)
 * each followed by a second image of the same matrix tiled as the 32x32x16 MFMA A operand,
 *   bf16 [rows/32][roundup(cols,16)/16][64 lanes][8]: lane (r = lane%32, half = lane/32) holds W[32*mi + r][16*ks + 8*half ..+7]
 * (one contiguous 1 KB wave load per k-step: the weights-stationary stage-5 kernel keeps it in registers).
 * x3d_pw_panel_elems(rows, cols) is the element count of BOTH images; always size panels with it.
 * `items` is an array in DEVICE memory; x3d_pw_panel_elems gives the element count of a panel. */
typedef struct {
  const float* w;              /* [Cout][Cin] fp32 */
  void* fwd_panel;
  void* dgrad_panel;
  int Cout, Cin;
} x3d_pw_pack_item;
long long x3d_pw_panel_elems(int rows, int cols);
int x3d_pw_pack_weights(const x3d_pw_pack_item* items, int n_items, int dtype /* X3D_BF16 or X3D_F16: element type of the panels */, void* stream);

/* weight gradient: dw [Cout][Cin] += sum_{n,p} dYraw[n][co][p] * act_in(x)[n][ci][q(p)] */
typedef struct {
  const void* g;
  const void* yraw;
  const float* coef;           /* as in dgrad */
  const void* x;               /* conv input [N][Cin][T][H][W] */
  const float* in_scale_shift; /* prologue of the forward pass, replayed */
  const float* in_gate;
  int in_act;
  float* dw;                   /* [Cout][Cin] += */
  int N, Cin, Cout, T, H, W, stride, dtype; /* T,H,W: INPUT extents (as in fwd) */
  float* dw_slab;              /* NULL | partial slabs instead of atomics, as x3d_pw_bwd_args.dw_slab: x3d_pw_wgrad_dw_parts(a) * Cout * Cin
                                * floats, every one of them written (dw untouched); added up by x3d_dw_slab_reduce / x3d_se_bnb_bwd */
  int dw_slab_parts;           /* the number of slabs dw_slab holds (x3d_pw_wgrad_dw_parts(a) when it was sized): checked against the grid */
  const x3d_bn_bwd_fold* coef_fold; /* NULL | derive `coef` from the BatchNorm-backward sums (x3d_bn_bwd_fold) */
} x3d_pw_wgrad_args;
int x3d_pw_wgrad(const x3d_pw_wgrad_args* a, void* stream);
int x3d_pw_wgrad_dw_parts(const x3d_pw_wgrad_args* a);   /* 0: the kernel behind this call has no slab form */

/* Which kernel instantiation a pointwise launch with these arguments runs ("pw_gemm_wst_kernel<1, 100, 6, 1, 27, 1>", ...),
 * without launching anything: the dispatch of x3d_pw_fwd / x3d_pw_dgrad / x3d_pw_wgrad / x3d_pw_bwd in dry-run mode (works
 * without a GPU; pointers are only inspected for alignment).  Exactly one struct is non-NULL.  Used by the dispatch-coverage
 * test (every instantiation the BASELINE configurations launch has an oracle-parity case) and by the profiling tools. */
int x3d_pw_kernel_name(const x3d_pw_fwd_args* fwd, const x3d_pw_dgrad_args* dgrad, const x3d_pw_wgrad_args* wgrad,
                       const x3d_pw_bwd_args* bwd, char* out, int cap);
/* 1: the kernel this call dispatches to takes coef_fold (x3d_bn_bwd_fold).  Exactly one struct is non-NULL. */
int x3d_pw_coef_fold_supported(const x3d_pw_dgrad_args* dgrad, const x3d_pw_wgrad_args* wgrad, const x3d_pw_bwd_args* bwd);

/* ------------------------------------------------------------------------------------------
 * K6  channelwise Conv3D(k=(3,3,3), s=(1,s,s), padding='same', groups=C, no bias)
 *     reference model.py:259-267.  TF-SAME (asymmetric) padding.  The HBM-bound headline kernel.
 *     Prologue on load: v = act(s*x + t) inside the image, 0 in the padding.
 *     Epilogue: stats [C][2] += ; pool [N][C] += sum over T,Ho,Wo of y (SE squeeze, model.py:277,312)
 *     DILATED form (x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil below; added under ABI 138 without a version bump: new symbols only,
 *     the argument structs are the dense ones): Conv3D(k=(3,3,3), strides 1, dilation_rate=(1,d,d), groups=C).  Padding d on
 *     each spatial side and 1 in time -- TF-SAME for the effective kernel 1 + 2d at stride 1, symmetric -- so y has x's extents.
 *     Prologue, epilogue and every backward output as in the dense form (csrc/dw_dil.hip).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* x;               /* [N][C][T][H][W] */
  const float* w;              /* [C][3][3][3] fp32 */
  void* y;                     /* [N][C][T][Ho][Wo] */
  const float* in_scale_shift; /* [C][2] or NULL */
  int in_act;
  double* stats;               /* [C][2] or NULL */
  double* pool;                /* [N][C] or NULL */
  int N, C, T, H, W, stride, dtype;
  const x3d_bn_fold* in_bn;    /* NULL, or: the prologue's scale/shift come from these statistics (in_scale_shift unused) */
} x3d_dw3d_fwd_args;
int x3d_dw3d_fwd(const x3d_dw3d_fwd_args* a, void* stream);

/* fused backward: dB = A*dv + B*braw + C with per-(n,c) coef_nc [N][C][4];
 *   ga = (conv^T dB) * [s_a*araw + t_a > 0]           -> [N][C][T][H][W]
 *   a_sums [C][2] += (sum ga, sum ga*araw) ; dw [C][27] += sum dB * relu(bn_a(araw))_padded */
typedef struct {
  const void* dv;              /* [N][C][T][Ho][Wo] */
  const void* braw;            /* [N][C][T][Ho][Wo] */
  const float* coef_nc;        /* [N][C][4] */
  const void* araw;            /* [N][C][T][H][W] */
  const float* a_scale_shift;  /* [C][2] */
  const float* w;              /* [C][27] */
  void* ga;                    /* [N][C][T][H][W] */
  double* a_sums;              /* [C][2] */
  float* dw;                   /* [C][27] */
  int N, C, T, H, W, stride, dtype;
} x3d_dw3d_bwd_args;
int x3d_dw3d_bwd(const x3d_dw3d_bwd_args* a, void* stream);
/* Which kernel instantiation a launch with these arguments runs ("dw3d_fwd_kernel<bf16, S, SW, NSV, CV>"),
 * without launching anything: the dispatch of x3d_dw3d_fwd / x3d_dw3d_bwd in dry-run mode.  Used by
 * bench.py so that its roofline row names the same kernel as the rocprofv3 summary.  Exactly one of
 * fwd / bwd is non-NULL.  Returns X3D_OK and a NUL-terminated string in out[0..cap). */
int x3d_dw3d_kernel_name(const x3d_dw3d_fwd_args* fwd, const x3d_dw3d_bwd_args* bwd, char* out, int cap);
/* The dilated form of K6: the same argument structs, the dilation d as an argument of its own.  d = 0 and d = 1 ARE the dense
 * conv: the call is handed to x3d_dw3d_fwd / x3d_dw3d_bwd as it stands.  d >= 2 needs stride == 1, d <= 4 and
 * (H + 2d)(W + 2d) <= 4096 (the zero-haloed plane of one channel must fit the LDS ring; no tiling); anything else is refused
 * with X3D_ERR_INVALID and a message naming the argument, before any launch.  x3d_dw3d_kernel_name_dil: the dry-run dispatch
 * of the two, as x3d_dw3d_kernel_name. */
int x3d_dw3d_fwd_dil(const x3d_dw3d_fwd_args* a, int dilation, void* stream);
int x3d_dw3d_bwd_dil(const x3d_dw3d_bwd_args* a, int dilation, void* stream);
int x3d_dw3d_kernel_name_dil(const x3d_dw3d_fwd_args* fwd, const x3d_dw3d_bwd_args* bwd, int dilation, char* out, int cap);

/* ------------------------------------------------------------------------------------------
 * K7/K8  squeeze-excite MLP: se_pool -> se_fc1(+bias, ReLU) -> se_fc2(+bias, sigmoid)
 *     reference model.py:274-290,311-315.  pool_sums [N][C] = sum over P points of braw (from K6);
 *     pooled = s_b * pool_sums / P + t_b.  gate [N][C], hidden [N][Wd] (saved for backward).
 * ------------------------------------------------------------------------------------------ */
int x3d_se_fwd(const double* pool_sums, double P, const float* b_scale_shift, const float* w1,
               const float* b1, const float* w2, const float* b2, float* gate, float* hidden, int N,
               int C, int Wd, void* stream);
/* backward of the SE branch + BN_b, from the per-(n,c) sums of x3d_pw_dgrad(EPI_SWISH_BWD):
 *   nc_sums [N][C][2] = (S1 = sum dv, S2 = sum dv*braw)
 *   dgate = s_b*S2 + t_b*S1 -> sigmoid' -> fc2^T -> relu' -> fc1^T -> dpool [N][C]
 *   dw1,db1,dw2,db2 += ; then BN_b backward over du = dv*gate + dpool/P:
 *   coef_nc [N][C][4] = (A*gate, B, C + A*dpool/P, 0) ; dgamma_b, dbeta_b += .
 * Without SE (w1 == NULL): gate = 1, dpool = 0.
 * P < 0: BN_b with frozen statistics (K3), |P| points per sample: coef_nc = (A*gate, +0, A*dpool/|P|, 0); the rest unchanged. */
typedef struct {
  const double* nc_sums;       /* [N][C][2] */
  const double* pool_sums;     /* [N][C] (forward) or NULL without SE */
  double P;                    /* points per sample; negative: frozen statistics */
  const float* b_scale_shift;  /* [C][2] */
  const float* b_mean_invstd;  /* [C][2] */
  const float* gamma_b;        /* [C] */
  const float* w1; const float* b1; const float* w2; const float* b2; /* SE params or NULL */
  const float* gate;           /* [N][C] or NULL */
  const float* hidden;         /* [N][Wd] or NULL */
  float* dw1; float* db1; float* dw2; float* db2;
  float* dgamma_b; float* dbeta_b;
  float* coef_nc;              /* out [N][C][4] */
  float* scratch;              /* N*(2*C + Wd) floats: dpool [N][C] | dz2 [N][C] | dz1 [N][Wd] */
  int N, C, Wd;
  x3d_dw_reduce_job reduce[2]; /* weight-gradient slabs of earlier x3d_pw_bwd launches, added up by extra workgroups of this launch */
} x3d_se_bnb_bwd_args;
int x3d_se_bnb_bwd(const x3d_se_bnb_bwd_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * K9  residual tail: Add + ReLU  (reference model.py:381-392)
 *     y = relu(s_c*c + t_c + shortcut), shortcut = s_r*r + t_r (conv shortcut) or x (identity);
 *     shortcut == NULL: y = relu(s_c*c + t_c)  (BN + ReLU after the stem, model.py:207-208)
 * ------------------------------------------------------------------------------------------ */
/* the same with the BatchNorm finalize of bn_c (and bn_r) folded in: see x3d_bn_fold */
int x3d_tail_fwd_bn(const void* c_raw, const x3d_bn_fold* c_bn, const void* shortcut, const x3d_bn_fold* r_bn,
                    void* y, int N, int C, long long P, int dtype, void* stream);
int x3d_tail_fwd(const void* c_raw, const float* c_scale_shift, const void* shortcut,
                 const float* r_scale_shift /* NULL: identity */, void* y, int N, int C, long long P,
                 int dtype, void* stream);
/* g = dy * [y > 0] written in place over dy; sums_c [C][2] += (sum g, sum g*c_raw);
 * if r_raw: sums_r [C][2] += (sum g, sum g*r_raw) */
int x3d_tail_bwd(void* dy_g, const void* y, const void* c_raw, const void* r_raw, double* sums_c,
                 double* sums_r, int N, int C, long long P, int dtype, void* stream);
/* K9d stochastic depth (drop-path) of the bottleneck branch, per sample: keep[n] is 0 (dropped) or 1 / (1 - rate) (kept).
 *     y = relu(keep[n] * (s_c*c + t_c) + shortcut); a dropped sample's c_raw is not loaded (y = relu(shortcut)).
 *     shortcut must not be NULL (the stem's BN + ReLU has no branch to drop). */
int x3d_tail_fwd_dp(const void* c_raw, const float* c_scale_shift, const void* shortcut,
                    const float* r_scale_shift /* NULL: identity */, const float* keep /* [N] */, void* y, int N, int C,
                    long long P, int dtype, void* stream);
/* g = dy * [y > 0] in place over dy (the shortcut path's gradient); g_branch = keep[n] * g rounded to the storage type (what
 * the `c` conv backward reads); sums_c [C][2] += (sum g_branch, sum g_branch*c_raw) over g_branch AS STORED; if r_raw:
 * sums_r [C][2] += (sum g, sum g*r_raw).  A dropped sample: g_branch = 0, c_raw not loaded, nothing added to sums_c. */
int x3d_tail_bwd_dp(void* dy_g, void* g_branch, const void* y, const void* c_raw, const void* r_raw, const float* keep,
                    double* sums_c, double* sums_r, int N, int C, long long P, int dtype, void* stream);
/* The keep table of one step, keep [L][N]: u = (Philox4x32-10(key = (seed_lo, seed_hi), counter = (step_lo, step_hi, l, n))[0]
 * >> 8) * 2^-24; keep[l][n] = u >= rates[l] ? 1.0f / (1.0f - rates[l]) : 0.  state (device, 4 x uint32: seed_lo, seed_hi,
 * step_lo, step_hi): the launch reads the 64-bit step, uses that one value for the whole table and stores step + 1 -- so the
 * same recorded launch draws a new table every step with no host involvement.  One workgroup; L * N <= 65536. */
int x3d_drop_path_draw(float* keep, const float* rates /* [L], device */, void* state, int L, int N, void* stream);
/* generic ReLU+BN backward reduce for stem / conv5: z = s*yraw + t.
 *   dy != NULL : g = dy * [z > 0]                (g may alias dy)
 *   dy == NULL : g = dpool[n][c] / P * [z > 0]   (global-average-pool backward, model.py:94,118)
 * sums [C][2] += (sum g, sum g*yraw).  g == NULL: sums only (the consumer applies the mask: x3d_dwt_bwd). */
int x3d_relu_bn_bwd_reduce(const void* dy, const float* dpool, const void* yraw,
                           const float* scale_shift, void* g, double* sums, int N, int C,
                           long long P, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * K5s even-pixel copy of a block input (ABI 133): dst [planes][ceil(H/2)][ceil(W/2)] = src [planes][H][W] at the even rows and
 *     columns, planes = N*C*T -- the pixels the stride-(1,2,2) 'valid' shortcut conv samples (reference model.py:360-367).
 *     With it the shortcut conv's forward, data gradient and weight gradient run as dense launches of x3d_pw_fwd /
 *     x3d_pw_bwd / x3d_pw_wgrad on the compact tensor (stride = 1, x_stride = 0) instead of the strided gathers.
 * ------------------------------------------------------------------------------------------ */
int x3d_subsample2(const void* src, void* dst, long long planes, int H, int W, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * K7/K10  head: pool5 (GlobalAveragePooling3D of relu(bn(conv5))), fc1 (1x1x1 conv on the pooled
 *     vector, no bias, ReLU), Dropout, fc2 Dense(+bias), Softmax(fp32), view mean.
 *     reference model.py:94-111,117-127
 * ------------------------------------------------------------------------------------------ */
int x3d_pool_fwd(const void* x_raw, const float* scale_shift, float* pooled /* [N][C] */, int N, int C,
                 long long P, int dtype, void* stream);
/* K7r  ROI head for action detection (PySlowFast DETECTION.ENABLE / ResNetRoIHead): per person box, the temporal mean of
 *     relu(bn(conv5)), ROIAlign and a spatial max -- detectron2 / torchvision roi_align(aligned=True) followed by MaxPool2d(R).
 *     The two launches take the places of x3d_pool_fwd and of x3d_relu_bn_bwd_reduce(dy == NULL, dpool).
 *   x_raw / yraw [N][C][T][H][W] in the storage dtype; scale_shift [C][2] fp32, as x3d_pool_fwd reads them.
 *   boxes [N][K][4] fp32 (x1, y1, x2, y2) in pixels of the clip; num_boxes [N] int32: slots k >= num_boxes[n] are empty.  K is
 *   a fixed capacity per clip: the boxes of sample n are rows n*K .. n*K+K-1 (no batch-index column; the backward is a gather).
 *   pooled [N*K][C] fp32; argmax [N*K][C] bytes, may be NULL in the forward (inference).
 * Forward:
 *   M[h][w] = mean_t relu(s_c*x + t_c), accumulated in fp32 (t in order).
 *   Box coordinates are multiplied by spatial_scale and clamped to [0, W] x [0, H] (x1', y1', x2', y2'), so the sample loops are
 *   bounded whatever the box is.  bin_w = (x2' - x1') / R, bin_h = (y2' - y1') / R; samples per bin gw = sampling_ratio > 0 ?
 *   sampling_ratio : ceil((x2' - x1') / R), gh likewise.  Sample (iy, ix) of bin (ph, pw) sits at
 *   y = y1' - 0.5 + ph*bin_h + (iy + 0.5)*bin_h/gh, x likewise (this geometry is worked out in fp64).
 *   Bilinear interpolation with border clamp: y <= 0 -> 0; y_low = floor(y) >= H-1 -> y_low = y_high = H-1, y = H-1.  After the
 *   box clamp no sample lies outside [-0.5, H-0.5], so torchvision's "outside -> 0" rule never applies.
 *   The bin value is the mean of its gh*gw samples; pooled = max over the R*R bins, argmax = the first maximal bin in row-major
 *   order (ph*R + pw).
 *   Treated as empty: an empty slot, a box with x2' <= x1' or y2' <= y1', any non-finite coordinate.  Such a slot gives
 *   pooled = 0, argmax = 0 and no gradient; the plane of a sample with num_boxes[n] <= 0 is not read.
 * Backward:
 *   dM[h][w] = sum over the boxes of sample n, in order, of dpooled[n*K+k][c] * (sum over the samples of the argmax bin of the
 *   bilinear weight of (h, w)) / (gh*gw);  g = round_to<T>(dM[h][w] / T * [s*yraw + t > 0]) for every t;
 *   sums [C][2] += (sum g, sum g*yraw), exactly as x3d_relu_bn_bwd_reduce with dy == NULL accumulates them.  dM is built without
 *   floating-point atomics (threads own pixels), so g is bit-reproducible; sums go through fp64 atomics like the sibling's.
 *   An argmax byte >= R*R is ignored (no gradient from that row).
 * Refused before any launch: H*W > 1024; R outside 1..15; K outside 1..64; N*K > 2048 (x3d_dense_bwd's limit on rows);
 *   sampling_ratio < 0; spatial_scale <= 0 or not finite. */
int x3d_roi_pool_fwd(const void* x_raw, const float* scale_shift, const float* boxes, const int* num_boxes,
                     float* pooled, unsigned char* argmax, int N, int C, int T, int H, int W, int K, int R,
                     int sampling_ratio, float spatial_scale, int dtype, void* stream);
int x3d_roi_pool_bwd(const float* dpooled, const unsigned char* argmax, const float* boxes, const int* num_boxes,
                     const void* yraw, const float* scale_shift, void* g, double* sums, int N, int C, int T, int H,
                     int W, int K, int R, int sampling_ratio, float spatial_scale, int dtype, void* stream);
/* y[n][m] = act( sum_k (x[n][k] * (mask ? mask[n][k]*mask_scale : 1)) * w[m][k] + b[m] ), all fp32 */
int x3d_dense_fwd(const float* x, const float* mask, float mask_scale, const float* w, const float* b,
                  float* y, int act, int N, int K, int M, void* stream);
/* dy is grad wrt the activated output y (ReLU only).  dx [N][K] (may be NULL), dw [M][K] +=, db [M] += */
int x3d_dense_bwd(const float* dy, const float* y, int act, const float* x, const float* mask,
                  float mask_scale, const float* w, float* dx, float* dw, float* db, int N, int K,
                  int M, void* stream);
/* probs = softmax(logits); loss_rows[n] = -log q_y + log sum_j q_j with q = clip(p,1e-7,1-1e-7)
 * (tf.keras SparseCategoricalCrossentropy on probabilities, train.py:104); dlogits = d(mean loss)/dlogits
 * scaled by grad_scale (= 1/global_batch).  labels int32; loss_rows / dlogits may be NULL.  A label outside
 * [0, M) is never used as an index: its loss row is NaN and its dlogits row zero. */
int x3d_softmax_xent(const float* logits, const int* labels, float* probs, float* loss_rows,
                     float* dlogits, float grad_scale, int N, int M, void* stream);
/* The same loss on dense target rows (ABI 137; label smoothing, mixup / CutMix): targets [N][M] fp32, y_j >= 0,
 * S = sum_j y_j.  loss_rows[n] = sum_j y_j * (-log q_j) + S * log sum_k q_k;
 * dL/dp_j = [1e-7 <= p_j <= 1-1e-7] * (-y_j / q_j + S / sum_k q_k), dlogits = grad_scale * p * (dL/dp - sum_k p_k dL/dp_k):
 * a one-hot row gives x3d_softmax_xent's result.  targets == NULL: probs only (loss_rows and dlogits must then be NULL);
 * loss_rows / dlogits may be NULL.  A NaN anywhere in a target row gives that row a NaN loss and a zero dlogits row.  One
 * workgroup per row, no atomics.  N * M < 2^31. */
int x3d_softmax_xent_soft(const float* logits, const float* targets, float* probs, float* loss_rows,
                          float* dlogits, float grad_scale, int N, int M, void* stream);
/* out[v][m] = mean over `views` consecutive rows (model.py:123-126) */
int x3d_view_mean(const float* probs, float* out, int videos, int views, int M, void* stream);
/* Keras metrics of a batch of probabilities (ABI 134; reference train.py:102-108 compile(metrics=[acc, top_5_acc]),
 * eval.py:48-66), added into four fp64 device counters:
 *   acc[0] += sum of loss rows, acc[1] += top-1 hits, acc[2] += top-k hits, acc[3] += N.
 * probs [N][M] fp32; labels [N] int32 (label_bytes 4) or int64 (label_bytes 8).  Per row, with q = clamp(p, 1e-7, 1-1e-7)
 * in fp64: loss = -log q_y + log sum_j q_j (NaN for a label outside [0, M), which is never used as an index);
 * top-k hit = label in range, every p_j finite and #{j : p_j > p_y} < k (tf.math.in_top_k: ties at the boundary hit);
 * top-1 hit = the same with no p_j > p_y and no j < y with p_j == p_y (first-index argmax).  One workgroup, no
 * floating-point atomics: the same inputs give bit-identical counters.  N * M < 2^31, k >= 1; N = 0 is a no-op. */
int x3d_topk_metrics(const float* probs, const void* labels, int label_bytes, double* acc, int N, int M, int k,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-label head (ABI 136; DATA.MULTI_LABEL): Dense(activation="sigmoid") + tf.keras.losses.BinaryCrossentropy().
 * ------------------------------------------------------------------------------------------ */
/* logits, targets [N][M] fp32, targets in [0, 1] (soft targets allowed).  probs = sigmoid(z).  Keras evaluates the loss on
 * a sigmoid output in its logits form [TF-3p]:  loss_rows[n] = mean_j ( max(z,0) - z*y + log1p(exp(-|z|)) ), the terms
 * and the row sum in fp64, stored as fp32;  dlogits = grad_scale * (sigmoid(z) - y) / M  (grad_scale = loss_scale /
 * global_batch, as for x3d_softmax_xent).  Finite for any finite z.  targets == NULL: probs only (loss_rows and dlogits
 * must then be NULL); loss_rows / dlogits may be NULL.  A NaN logit gives its row a NaN loss and its own dlogits element
 * NaN.  One launch (one workgroup per row), no atomics.  N * M < 2^31. */
int x3d_sigmoid_bce(const float* logits, const float* targets, float* probs, float* loss_rows, float* dlogits,
                    float grad_scale, int N, int M, void* stream);
/* out[v][m] = max over `views` consecutive rows (the "max" TEST.ENSEMBLE_METHOD); a NaN in any view gives NaN */
int x3d_view_max(const float* probs, float* out, int videos, int views, int M, void* stream);
/* Per-class average precision over an evaluation set (sklearn.metrics.average_precision_score).  scores, targets [N][M]
 * fp32; ap double[M]; npos int[M].  Per class c, with positives = {i : targets[i][c] >= 0.5} and P = their number:
 *   ap[c] = (1/P) * sum over positives i of TP(s >= s_i) / #{j : s_j >= s_i},   TP(s >= t) = #{positives with s >= t}
 * Equal scores form one threshold (ties included exactly; -0 equals +0).  npos[c] = P.  P == 0: ap[c] = NaN (mAP drops
 * the class); any NaN score in the column: ap[c] = NaN.  All counts are integers; the sum is fp64 in a fixed order with
 * no floating-point atomics, so the same inputs give bit-identical ap.  One workgroup per class, O(N log P).
 * Limits: N * M < 2^31 (refused otherwise); at most X3D_AP_MAX_POSITIVES positives per class -- a column with more is
 * never truncated: its ap is NaN and npos[c] = -P (only possible when N > X3D_AP_MAX_POSITIVES). */
#define X3D_AP_MAX_POSITIVES 32768
int x3d_multilabel_ap(const float* scores, const float* targets, int N, int M, double* ap, int* npos, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frame-mAP for action detection (AVA; the PASCAL evaluator of the TensorFlow object-detection API, restated): the proposals
 * of an image are matched against its annotated boxes per class, and the per-class AP is PASCAL VOC's area under the monotone
 * precision envelope.  Where the original leaves something to chance (score ties) the rules below pin it.
 *   Sizes: I images, K proposal slots and G ground-truth slots per image (1 <= K, G <= 64), C classes.
 *   scores [I*K][C] fp32 (row i*K + k); boxes [I][K][4] fp32 (x1, y1, x2, y2), num_boxes [I] int32;
 *   gt_boxes [I][G][4] fp32, num_gt [I] int32; gt_labels [I][G][C] bytes, non-zero = box g carries class c (several allowed).
 * Validity: a proposal is a DETECTION iff k < num_boxes[i], its four coordinates are finite, x2 > x1 and y2 > y1 (the ROI
 *   head's "treated as empty" rule, negated); a ground-truth box is VALID by the same rule with num_gt.  What an empty or invalid
 *   slot holds -- box, score, labels -- is never used.
 * IoU, in IEEE double from the fp32 coordinates, every operation rounded on its own (no fused multiply-add), the division
 *   correctly rounded:  iw = max(0, min(ax2, bx2) - max(ax1, bx1)), ih likewise;  inter = iw * ih;
 *   ua = (ax2 - ax1) * (ay2 - ay1), ub likewise;  iou = inter / (ua + ub - inter).  This is numpy's value bit for bit, so every
 *   decision below is exact.
 * Matching, per image i, class c and detection d:
 *   1. among the valid ground-truth boxes with gt_labels[i][g][c] != 0 (none: d is a false positive), g*(d) is the one with the
 *      largest iou(d, g), the lowest g among equals; d is a CANDIDATE iff iou(d, g*(d)) >= iou_threshold.  Only the arg-max box
 *      is tried: a detection whose best box is claimed is a false positive even if another box of the class would pass.
 *   2. the detections of the image are ordered by score descending, the lower slot k first among equal scores; d is a TRUE
 *      POSITIVE iff it is a candidate and no detection before it in that order is a candidate with the same g*.
 *   3. a detection whose score for c is NaN is never a candidate and claims nothing.
 * x3d_frame_match writes tp [I*K][C] bytes (1 / 0; 0 for a non-detection) and det_scores [I*K][C] fp32 (the score of a
 *   detection unchanged, NaN included; -inf for a non-detection), and INCREMENTS ngt [C] int32 by the number of valid
 *   ground-truth boxes carrying c (integer atomics: the result does not depend on their order).  One workgroup per image, the
 *   IoU table in LDS, one wave per class; no floating-point atomics, nothing else written that another workgroup writes.
 *   Refused before the launch: a null pointer; I < 1; K or G outside 1..64; C < 1; I*K*C >= 2^31; iou_threshold NaN or outside
 *   (0, 1].
 * x3d_frame_ap, per class c over the N = I*K rows of a whole evaluation set: order [N][C] int64 holds the class's row
 *   permutation by det_scores[:, c] descending, equal scores by row index ascending (a stable sort; the original's argsort is
 *   unstable), NaN scores first -- what torch.sort(descending=True, stable=True) returns.  With the true positives t = 1..P in
 *   that order and pos_t the 1-based position of the t-th:  prec_t = t / pos_t;  env_t = max over t' >= t of prec_t';
 *   ap[c] = (sum over t of env_t) / ngt[c] in double;  ntp[c] = P.  Rows at -inf sort behind every detection and carry tp = 0.
 *   ngt[c] <= 0: ap[c] = NaN (the class is dropped from the mean).  ngt[c] > 0 and P == 0: ap[c] = 0.  A NaN among the class's
 *   scores (the class's first row in `order`): ap[c] = NaN.  An entry of `order` outside [0, N) is never followed (its
 *   position counts as a false positive).  One workgroup per class; the flags stream from memory, so there is no cap on rows
 *   or true positives per class; the sums are added in a fixed order: the same inputs give the same bits.
 *   Refused before the launch: a null pointer; N < 1; C < 1; N*C >= 2^31. */
int x3d_frame_match(const float* scores, const float* boxes, const int* num_boxes, const float* gt_boxes,
                    const unsigned char* gt_labels, const int* num_gt, int I, int K, int G, int C, double iou_threshold,
                    unsigned char* tp, float* det_scores, int* ngt, void* stream);
int x3d_frame_ap(const unsigned char* tp, const float* det_scores, const long long* order, const int* ngt, int N, int C,
                 double* ap, int* ntp, void* stream);

/* ------------------------------------------------------------------------------------------
 * Knowledge distillation (DISTILL.* of the config): the three training losses with a second term against a teacher's
 * logits at a temperature (Hinton, Vinyals, Dean 2015).  logits, teacher_logits [N][M] fp32.  With z = logits,
 * t = teacher_logits, T = temperature, a = alpha, u = z / T and v = t / T:
 *   loss_rows[n] = (1 - a) * hard + a * kd;   kd_rows[n] = kd (unweighted; may be NULL);
 *   dlogits = grad_scale * ((1 - a) * d hard / dz + a * d kd / dz)      (grad_scale = loss_scale / global_batch).
 * probs is the T = 1 output of the head the hard term belongs to, bit-identical to that kernel's (the training metrics
 * read it); loss_rows / dlogits may be NULL.
 * alpha == 0: the teacher is not read (teacher_logits may be NULL), loss_rows and dlogits are bit-identical to the hard
 * kernel's and kd_rows is 0 -- a branch, not a product with 0.
 * A teacher logit that is not finite (NaN, +-inf) anywhere in a row: loss_rows[n] and kd_rows[n] are NaN and the dlogits
 * row is zero (an unusable sample, as for a label outside [0, M)); probs is written all the same.  The hard term's own
 * rules for such samples (below) hold whatever the teacher says; kd_rows[n] is then still the row's KD term.
 * Refused before any launch (X3D_ERR_INVALID, the message names the argument): logits or probs NULL; alpha outside [0, 1]
 * or NaN; temperature not finite or <= 0; alpha > 0 with teacher_logits NULL; N <= 0 or M <= 0; N * M >= 2^31;
 * teacher_logits or targets sharing a byte with probs, loss_rows, kd_rows or dlogits.
 * One launch, one 256-thread workgroup per row, sums in a fixed order, no atomics.
 * ------------------------------------------------------------------------------------------ */
/* Softmax head.  Exactly one of labels ([N] int32: the hard term of x3d_softmax_xent, a label outside [0, M) gives a NaN
 * loss row and a zero dlogits row) and targets ([N][M] fp32 dense rows: that of x3d_softmax_xent_soft, likewise for a NaN
 * target) must be given; both or neither is refused.
 *   kd = T^2 * sum_j p_t,j * (log p_t,j - log p_s,j),   log p_s = u - lse(u), log p_t = v - lse(v), p_t = exp(log p_t):
 * evaluated in log space and in fp64, no clipping; a teacher probability that underflows to 0 contributes 0, never NaN.
 *   d kd / dz = T * (softmax(u) - softmax(v)). */
int x3d_softmax_xent_kd(const float* logits, const float* teacher_logits, const int* labels, const float* targets,
                        float* probs, float* loss_rows, float* kd_rows, float* dlogits, float grad_scale, float alpha,
                        float temperature, int N, int M, void* stream);
/* Sigmoid head (DATA.MULTI_LABEL): the hard term of x3d_sigmoid_bce on targets [N][M] fp32 (required).  The KD term is the
 * Bernoulli KL per class against sigmoid(v), >= 0 and 0 where z = t:
 *   kd = T^2 * mean_j [ (softplus(u_j) - sigmoid(v_j) u_j) - (softplus(v_j) - sigmoid(v_j) v_j) ],
 *   softplus(x) = max(x, 0) + log1p(exp(-|x|)); the terms and the row sum in fp64, as the hard term's.
 *   d kd / dz_j = T * (sigmoid(u_j) - sigmoid(v_j)) / M. */
int x3d_sigmoid_bce_kd(const float* logits, const float* teacher_logits, const float* targets, float* probs,
                       float* loss_rows, float* kd_rows, float* dlogits, float grad_scale, float alpha, float temperature,
                       int N, int M, void* stream);

/* ------------------------------------------------------------------------------------------
 * Class-imbalance losses (LOSS.* of the config): class weights, a positive weight, sample weights and focal factors on the
 * hard term of either head, one entry point per head; each covers labels, dense targets and distillation.
 * class_w, pos_w [M] fp32 and row_w [N] fp32 may each be NULL = all ones; below c = class_w, w+ = pos_w, r = row_w.
 *   loss_rows[n] = (1 - a) * hard + a * r_n * kd;   kd_rows[n] = kd, the unweighted KD term (0 with alpha == 0);
 *   dlogits = grad_scale * d loss_rows / dz.   The class and positive weights and the focal factors act on `hard` only.
 * alpha, temperature, teacher_logits, kd: the distillation block above, rule for rule (alpha == 0 does not read the teacher,
 * which may then be NULL; a non-finite teacher logit makes the row unusable).  probs is bit-identical to the plain kernel's.
 * p, the row maximum and the softmax sum are the fp32 values of the plain kernels; everything behind them is evaluated in
 * fp64 and stored as fp32.
 * Bit rule: with class_w, pos_w and row_w NULL and every gamma 0 the entry points launch the distillation kernels of the
 * block above (whose alpha == 0 branch runs the plain kernels' statements): every output has the bits of x3d_softmax_xent_kd
 * / x3d_sigmoid_bce_kd, and at alpha == 0 those of x3d_softmax_xent / x3d_softmax_xent_soft / x3d_sigmoid_bce.
 * Unusable rows -- a label outside [0, M), a NaN target, a non-finite teacher logit (alpha > 0), a row_w[n] that is NaN,
 * negative or infinite -- get a NaN loss row and a zero dlogits row.  row_w[n] == 0 is a valid row: loss 0, gradient 0.
 * Refused before any launch (X3D_ERR_INVALID, the message names the argument): what the distillation block refuses; a gamma
 * that is negative, NaN, infinite or above 8; class_w, pos_w or row_w sharing a byte with probs, loss_rows, kd_rows or
 * dlogits.  The values of class_w and pos_w are the caller's to check (config.loss_settings does: finite, >= 0).
 * One launch, one 256-thread workgroup per row, sums in a fixed order, no atomics.
 * ------------------------------------------------------------------------------------------ */
/* Softmax head.  Exactly one of labels ([N] int32, the one-hot row y) and targets ([N][M] fp32 dense rows y) is given.
 * With q = clip(p, 1e-7, 1 - 1e-7), x_j = q_j / sum_k q_k and f(x) = (1 - x)^gamma * (-log x):
 *   hard = r_n * sum_j c_j y_j f(x_j)
 * -- Keras CategoricalFocalCrossentropy with a per-class alpha; gamma = 0 with labels: Keras class_weight, c_y * the plain
 * loss; gamma = 0, c = r = 1: the loss of x3d_softmax_xent / _soft.  With a_j = r_n c_j y_j:
 *   dL/dp_k = [1e-7 <= p_k <= 1 - 1e-7] * (a_k f'(x_k) - sum_j a_j f'(x_j) x_j) / sum q,
 *   d hard / dz = p * (dL/dp - sum_k p_k dL/dp_k).
 * x = 1 (possible only at M = 1): loss 0, gradient 0, never NaN. */
int x3d_softmax_xent_w(const float* logits, const float* teacher_logits, const int* labels, const float* targets,
                       const float* class_w, const float* row_w, float* probs, float* loss_rows, float* kd_rows,
                       float* dlogits, float grad_scale, float gamma, float alpha, float temperature, int N, int M,
                       void* stream);
/* Sigmoid head (DATA.MULTI_LABEL); targets [N][M] fp32 (required).  With s = sigmoid(z):
 *   hard = r_n * mean_j c_j [ y_j w+_j (1 - s_j)^gamma_pos softplus(-z_j) + (1 - y_j) s_j^gamma_neg softplus(z_j) ]
 * -- torch BCEWithLogitsLoss(pos_weight) at gamma 0, Keras BinaryFocalCrossentropy at gamma_pos == gamma_neg, asymmetric
 * focusing (without the probability margin) otherwise; linear in y, so soft targets are defined; everything off:
 * softplus(z) - z y, the loss of x3d_sigmoid_bce.  dlogits is the exact derivative:
 *   d/dz (1 - s)^g softplus(-z) = -(1 - s)^g (g s softplus(-z) + 1 - s),   d/dz s^g softplus(z) = s^g (g (1 - s) softplus(z) + s). */
int x3d_sigmoid_bce_w(const float* logits, const float* teacher_logits, const float* targets, const float* class_w,
                      const float* pos_w, const float* row_w, float* probs, float* loss_rows, float* kd_rows,
                      float* dlogits, float grad_scale, float gamma_pos, float gamma_neg, float alpha, float temperature,
                      int N, int M, void* stream);
/* Per-class top-1 counters (mean per-class accuracy): for every row with a label in [0, M), counts[y] += 1, and hits[y] += 1
 * where the row is a top-1 hit by x3d_topk_metrics's rule (first-index argmax, every p_j finite).  A label outside [0, M) is
 * counted nowhere.  hits, counts: int64 [M] device counters that are added into (zero them first).  probs [N][M] fp32;
 * labels [N] int32 (label_bytes 4) or int64 (8).  Integer atomics only: the same inputs give the same counters.
 * N * M < 2^31; N = 0 is a no-op. */
int x3d_class_hits(const float* probs, const void* labels, int label_bytes, long long* hits, long long* counts, int N,
                   int M, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mixup / CutMix (ABI 137; MIXUP.* of the config): a batch mixed with its own reverse, clip i with clip N-1-i.
 * ------------------------------------------------------------------------------------------ */
#define X3D_MIX_MIXUP 1
#define X3D_MIX_CUTMIX 2
/* x, out: channels-last clip batches [N][T][H][W][C] of storage type dtype (X3D_F32 / X3D_BF16 / X3D_F16), contiguous.
 *   X3D_MIX_MIXUP:  out_i = lam * x_i + (1 - lam) * x_{N-1-i} for every element: fp32 arithmetic on the stored values, one
 *                   round-to-nearest-even to the storage type.  lam = 1 returns x and lam = 0 the reversed batch, bit for bit.
 *   X3D_MIX_CUTMIX: the box [y0, y1) x [x0, x1) of every frame of clip i is replaced by the same box of clip N-1-i, everything
 *                   else is copied: bit-exact (lam is checked but not used; an empty box returns x).
 * out may equal x (in place: one thread owns both ends of a pair, so no second copy of the batch exists; CutMix then touches
 * the box only) or be a buffer that does not overlap it.  With odd N the middle clip is its own partner and comes out
 * bit-identical.  Any alignment of the element type is accepted; every offset is 64-bit.
 * Refused: null pointers, non-positive extents, N > 131070, an unknown mode or dtype, lam outside [0, 1] or not finite, for
 * CutMix a box that is not inside the frame (0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W), out overlapping x without being
 * equal to it.  Nothing is written then. */
int x3d_mix_clips(const void* x, void* out, int mode, float lam, int y0, int y1, int x0, int x1, int N, int T, int H, int W,
                  int C, int dtype, void* stream);
/* The soft targets of a mixed batch, out [N][M] fp32 (fp64 arithmetic, rounded once).  Exactly one of labels / targets:
 *   labels [N] int32:     s(c)_j = (1 - eps) * [j == c] + eps / M;  out_i = lam * s(label_i) + (1 - lam) * s(label_{N-1-i}),
 *                         0 <= eps < 1.  A label outside [0, M) is never used as an index: its row and its partner's row are
 *                         all NaN.  hard [N] int32 (may be NULL) = the class the training metrics count against: label_i if
 *                         lam >= 0.5, else label_{N-1-i}; a buffer of its own, not `labels`.
 *   targets [N][M] fp32:  out_i = lam * t_i + (1 - lam) * t_{N-1-i};  out may equal targets (in place) or must not overlap
 *                         it; eps must be 0 and hard NULL.
 * The middle row of an odd batch is s(label) / t itself.  One workgroup per pair.  N * M < 2^31. */
int x3d_mix_targets(const int* labels, const float* targets, float* out, int* hard, float lam, float eps, int N, int M,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * K12  SGD with Nesterov momentum + L2 (train.py:89-92, model.py:47):
 *     g' = g + 2*wd*w (where l2_mask) ; v = m*v - lr*g' ; w = w + m*v - lr*g'
 *     flat fp32 arrays of n elements; wd_mask [n] in {0,1} as uint8 (NULL: no decay)
 * ------------------------------------------------------------------------------------------ */
int x3d_sgd_nesterov(float* w, float* v, const float* g, const unsigned char* l2_mask, float lr,
                     float momentum, float weight_decay, float grad_scale, long long n, void* stream);
/* Adam, the reference's other optimizer branch (tf.optimizers.Adam(learning_rate), train.py:93-95; Keras defaults
 * beta1 0.9, beta2 0.999, eps 1e-7):  g' as above; m = b1*m + (1-b1)*g'; v = b2*v + (1-b2)*g'^2;
 * w -= lr * sqrt(1 - b2^step) / (1 - b1^step) * m / (sqrt(v) + eps).  `step` counts from 1. */
int x3d_adam(float* w, float* m, float* v, const float* g, const unsigned char* l2_mask, float lr, float beta1,
             float beta2, float eps, float weight_decay, float grad_scale, long long step, long long n, void* stream);
/* ------------------------------------------------------------------------------------------
 * The solver step around K12 (SOLVER.* of the config): global-norm gradient clipping, gradient accumulation
 * and an exponential moving average (EMA) of the weights, decided and applied on the device.  Added under ABI 138 without a
 * version bump: new symbols only, no existing prototype, struct or constant changed.  No floating-point atomics.
 *
 * x3d_grad_sumsq: out[0] = sum over i of (double)g[i]^2, squared and accumulated in fp64; the per-workgroup partials are
 *     added in a fixed ascending order, so the same input gives the same bits on every run.  out[1] = the number of
 *     non-finite g[i] (as a double; 0.0 = all finite); those entries add nothing to out[0].  Two launches (partials, final
 *     sum); nothing allocates or synchronises.  scratch: x3d_grad_sumsq_scratch(n) doubles of device memory, the caller's
 *     (a fixed function of n: twice the partial count); it need not be zeroed.
 * x3d_sgd_nesterov_ex / x3d_adam_ex: x3d_sgd_nesterov / x3d_adam with
 *     norm: NULL, or the out[2] of x3d_grad_sumsq over the same g.  The gradient is multiplied by
 *           c = grad_scale * min(1, max_norm / (sqrt(norm[0]) * grad_scale + 1e-6))
 *           instead of grad_scale: torch.nn.utils.clip_grad_norm_'s rule on the UNSCALED gradient g * grad_scale; computed
 *           on the device in fp64 and rounded once (no clipping: exactly grad_scale).  If norm[1] != 0 the launch writes
 *           NOTHING: w, the slots and ema stay bit for bit, the step is skipped.
 *     ema:  NULL, or [n]: ema[i] = ema_decay * ema[i] + (1 - ema_decay) * w_new[i] in the same pass, evaluated as
 *           ema[i] + (1 - ema_decay) * (w_new[i] - ema[i]) (w == ema is a fixed point).
 *     norm == NULL and ema == NULL: bit-identical to x3d_sgd_nesterov / x3d_adam -- the update arithmetic is one device
 *     function both call.  16-byte aligned arrays (l2_mask 4-byte) move as 16-byte vectors, anything else by element.
 * x3d_ema_update: the same EMA rule over n floats the optimizer does not own (the BatchNorm moving statistics behind the
 *     trainable block).  norm: NULL, or skip when norm[1] != 0.
 * x3d_grad_accum: acc = g (first != 0) or acc += g, exact fp32.  acc may be g itself (acc = 2 g).
 * Refused before any launch (X3D_ERR_INVALID): a null required pointer, n <= 0, max_norm <= 0 or not finite with norm, a
 * decay outside [0, 1) with ema (x3d_ema_update: always), a float pointer that is not 4-byte aligned.
 * ------------------------------------------------------------------------------------------ */
long long x3d_grad_sumsq_scratch(long long n);
int x3d_grad_sumsq(const float* g, long long n, double* scratch, double* out, void* stream);
int x3d_sgd_nesterov_ex(float* w, float* v, const float* g, const unsigned char* l2_mask, float lr, float momentum,
                        float weight_decay, float grad_scale, const double* norm, float max_norm,
                        float* ema, float ema_decay, long long n, void* stream);
int x3d_adam_ex(float* w, float* m, float* v, const float* g, const unsigned char* l2_mask, float lr, float beta1, float beta2,
                float eps, float weight_decay, float grad_scale, long long step, const double* norm, float max_norm,
                float* ema, float ema_decay, long long n, void* stream);
int x3d_ema_update(float* ema, const float* w, float decay, const double* norm, long long n, void* stream);
int x3d_grad_accum(float* acc, const float* g, long long n, int first, void* stream);
/* ------------------------------------------------------------------------------------------
 * Layer-wise optimizers on the flat buffers: LARS, AdamW, LAMB (TRAIN.OPTIMIZER = lars | adamw | lamb, OPTIM.* of the config,
 * INTEGRATION.md).  Added under ABI 138 without a version bump: new symbols only.  No floating-point atomics; a fixed number
 * of launches whatever the number of tensors; nothing allocates or synchronises.
 *
 * SEGMENTS AND THE CHUNK TABLE.  A segment t is one trainable tensor of the flat buffers (offset, length); what lies between
 * segments is padding and is never read or written, in w, the slots or ema.  The walk is driven by two int32 tables in DEVICE
 * memory, built once on the host (x3d_tf_amd/segments.py):
 *     chunks [nchunk][3] = (segment, first element, count): X3D_SEG_CHUNK elements at most, inside ONE segment, the chunks of a
 *                          segment adjacent and ascending; first % 4 == 0 (segment offsets are 16-byte aligned); every element
 *                          of every segment in exactly one chunk.  Elements are indexed with int: buffers under 2^31 elements.
 *     segs   [nseg][3]   = (first chunk, number of chunks, l2 flag) -- l2_t = ParamSpec.l2: conv / dense kernels.
 * One wave takes one chunk: count / 4 vectors of 16 bytes 64 lanes wide (base pointers that are not 16-byte aligned: the same
 * elements by the same lanes, loaded one by one), then the count % 4 last elements by lanes 0..2.  Sums: a lane adds its
 * elements in ascending order in fp64, the 64 lanes by a fixed butterfly -> one partial per chunk; a segment's partials are then
 * added by one wave in a fixed order.  The same inputs give the same bits on every run and on either alignment path.
 *
 * x3d_seg_sumsq: out[t] = sum over the segment of (double)a[i]^2.  partials: nchunk doubles of scratch.  Two launches.
 *
 * c below = the coefficient of the _ex launches: grad_scale, or with norm grad_scale * min(1, max_norm / (sqrt(norm[0]) *
 * grad_scale + 1e-6)); norm[1] != 0: EVERY launch of the call writes nothing -- w, the slots, ema and q stay bit for bit.
 * ||.|| = sqrt of the fp64 segment sum.  q [nseg] fp32 is written to device memory: computed in fp64 from the fp64 sums and
 * the fp32 arguments, rounded to fp32 once.  g is read-only.  ema / ema_decay as in the _ex launches, written by the last pass.
 *
 * x3d_lars (slot v): lambda = 2 * weight_decay, eta = trust_coef
 *     l2_t and ||w_t|| > 0 and ||g_t|| > 0: q_t = eta ||w_t|| / (c ||g_t|| + lambda ||w_t|| + eps); clip != 0: q_t = min(q_t / lr, 1)
 *     otherwise q_t = 1
 *     g' = q_t (c g + [l2_t] lambda w) ; v = mom v - lr g' ; w = w + mom v - lr g'
 *     roundings: c g | FMA (2 wd) w + . (where l2_t) | . * q_t | then x3d_sgd_nesterov's sequence on g' (lr g', FMA mom v - .,
 *     FMA mom v' + w, FMA -lr g' + .).  q_t = 1: bit-identical to x3d_sgd_nesterov_ex on the segment (its mask = l2_t).
 *     Launches: partial sums of w and g (partials: 2 * nchunk doubles), q, apply.
 * x3d_adamw (slots m, v): x3d_adam_ex's step with the coupled L2 term off, then, where l2_t and decay > 0,
 *     w = FMA(-(lr * decay), w_old, w_adam) (lr * decay rounded once; w_old = w before the step).  decay = 0: bit-identical to
 *     x3d_adam_ex with weight_decay = 0 on every segment.  One launch.
 * x3d_lamb (slots m, v): r = (float)(sqrt(1 - beta2^step) / (1 - beta1^step)) (fp64 on the host)
 *     m = b1 m + (1 - b1) c g ; v = b2 v + (1 - b2) (c g)^2                     (x3d_adam's expressions and roundings)
 *     u = r m / (sqrt(v) + eps) + [l2_t] decay w
 *     l2_t and ||w_t|| > 0 and ||u_t|| > 0: q_t = ||w_t|| / ||u_t||, otherwise q_t = 1 ;  w = w - lr q_t u
 *     roundings of u: r m | sqrt v | . + eps | the quotient | FMA decay w + . (where l2_t); of w: lr q_t | FMA -(lr q_t) u + w.
 *     Launches: m, v and the partial sums of w and u (partials: 2 * nchunk doubles); q; apply, which recomputes u from the
 *     m, v the first pass wrote (u is never stored).
 * Refused before any launch (X3D_ERR_INVALID): a null required pointer, nchunk <= 0, nseg <= 0, a float pointer that is not
 * 4-byte or a double pointer that is not 8-byte aligned, trust_coef <= 0, eps < 0 (x3d_lamb: <= 0), decay < 0, any of them not
 * finite, step < 1, and what the _ex launches refuse of norm / max_norm / ema_decay.
 * ------------------------------------------------------------------------------------------ */
#define X3D_SEG_CHUNK 1024
int x3d_seg_sumsq(const float* a, const int* chunks, int nchunk, const int* segs, int nseg, double* partials, double* out,
                  void* stream);
int x3d_lars(float* w, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg, float lr,
             float momentum, float weight_decay, float grad_scale, float trust_coef, float eps, int clip, const double* norm,
             float max_norm, float* ema, float ema_decay, double* partials, float* q, void* stream);
int x3d_adamw(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg, float lr,
              float beta1, float beta2, float eps, float decay, float grad_scale, long long step, const double* norm,
              float max_norm, float* ema, float ema_decay, void* stream);
int x3d_lamb(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg, float lr,
             float beta1, float beta2, float eps, float decay, float grad_scale, long long step, const double* norm,
             float max_norm, float* ema, float ema_decay, double* partials, float* q, void* stream);
/* ------------------------------------------------------------------------------------------
 * Fine-tuning: frozen tensors and per-tensor learning rates (SOLVER.FREEZE / LR_MULT / LAYER_DECAY of the config,
 * x3d_tf_amd/finetune.py).  Added under ABI 138 without a version bump: new symbols only; every entry point
 * above keeps its signature and its bits.  All five rules and the gradient reduction walk a chunk table (above) built from the
 * TUNED tensors only: a frozen tensor is in no chunk, so its weights, slots and ema are never read and never written -- whatever
 * its gradient holds -- and its gradient is in neither the norm nor the finite count.  (A learning rate of 0 would not do that:
 * Nesterov momentum still moves w, and 0 * inf is NaN.)
 *
 *     lr_scale: NULL (every scale 1), or [nseg] fp32 in device memory, > 0 and finite (the caller's to see to).  The learning
 *               rate of segment t is lr_t = lr * lr_scale[t], ONE fp32 product, read once per chunk, and it stands wherever the
 *               rule has lr: both uses in the Nesterov step and the LARC clip min(q_t / lr_t, 1) (sgd, lars); the bias-corrected
 *               (float)((double)lr_t * sqrt(1 - beta2^step) / (1 - beta1^step)) and ld = lr_t * decay (adam, adamw); lr_t q_t
 *               (lamb).  The update of segment t therefore has the bits of the plain update at the learning rate fl32(lr *
 *               lr_scale[t]).
 *     norm / max_norm / ema / ema_decay: as in the entry point of the same rule, and refused alike.
 *
 * x3d_seg_grad_sumsq: x3d_grad_sumsq over the table's chunks -- out[0] = the fp64 sum of squares of the finite g[i] inside
 *     them, out[1] = the number of non-finite ones (as a double); every `norm` above can be this out[2].  One partial sum and
 *     one count per chunk (partials: 2 * nchunk doubles; a lane adds its elements in ascending order, the lanes by a fixed
 *     butterfly), then one launch that adds them in ascending order: no atomics, the same bits on every run and on either
 *     alignment path.  Two launches.
 * x3d_sgd_pt / x3d_adam_pt: x3d_sgd_nesterov_ex / x3d_adam_ex on the chunk walk; the l2 flag is segs[t][2], not a byte mask.
 *     One launch each.
 * x3d_lars_pt / x3d_adamw_pt / x3d_lamb_pt: x3d_lars / x3d_adamw / x3d_lamb -- the same three / one / three launches of the
 *     same kernels, instantiated with lr_t per segment.  q [nseg] is in the order of the table's segments.
 * lr_scale == NULL (or all 1) and a table over all segments: bit-identical to the entry point of the same rule (for sgd / adam:
 *     on every segment, with its mask = l2_t).  Refused before any launch: what that entry point refuses, and an lr_scale that
 *     is not 4-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int x3d_seg_grad_sumsq(const float* g, const int* chunks, int nchunk, const int* segs, int nseg, double* partials, double* out,
                       void* stream);
int x3d_sgd_pt(float* w, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
               const float* lr_scale, float lr, float momentum, float weight_decay, float grad_scale, const double* norm,
               float max_norm, float* ema, float ema_decay, void* stream);
int x3d_adam_pt(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                const float* lr_scale, float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                long long step, const double* norm, float max_norm, float* ema, float ema_decay, void* stream);
int x3d_lars_pt(float* w, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                const float* lr_scale, float lr, float momentum, float weight_decay, float grad_scale, float trust_coef,
                float eps, int clip, const double* norm, float max_norm, float* ema, float ema_decay, double* partials, float* q,
                void* stream);
int x3d_adamw_pt(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                 const float* lr_scale, float lr, float beta1, float beta2, float eps, float decay, float grad_scale,
                 long long step, const double* norm, float max_norm, float* ema, float ema_decay, void* stream);
int x3d_lamb_pt(float* w, float* m, float* v, const float* g, const int* chunks, int nchunk, const int* segs, int nseg,
                const float* lr_scale, float lr, float beta1, float beta2, float eps, float decay, float grad_scale,
                long long step, const double* norm, float max_norm, float* ema, float ema_decay, double* partials, float* q,
                void* stream);
/* LossScaleOptimizer support (Keras mixed_float16, train.py:99-100): *flag (device int the caller set to 1) is cleared
 * when any of the n values is inf / nan -- the step is then skipped and the loss scale halved. */
int x3d_all_finite(const float* g, long long n, int* flag, void* stream);
/* ------------------------------------------------------------------------------------------
 * The fp16 loss scaler on the device (SOLVER.DEVICE_LOSS_SCALE of the config): Keras' dynamic LossScaleOptimizer
 * without a host read in the training step.  Added under ABI 138 without a version bump: new symbols only.  Plain vector loads
 * and stores, no atomics; nothing allocates or synchronises.
 *
 * STATE: X3D_LOSS_SCALE_STATE doubles of device memory, 8-byte aligned, the caller's:
 *     [0] the scale S, a power of two >= 1        [1] 1 / S (kept equal to it by x3d_loss_scale_update)
 *     [2] consecutive finite steps                [3] skipped steps, total
 *     [4] applied steps, total                    [5] 1.0 if the last update was skipped, else 0.0
 *     [6], [7] zero
 *   The counters are whole numbers held as doubles: exact up to 2^53.
 *
 * x3d_loss_scale_apply: x[i] = x[i] * (float)state[0], one fp32 product.  Launched on the head's dlogits, with the head given
 *     1 / global_batch instead of S / global_batch: the head kernels are linear in that factor and S is a power of two, so the
 *     backward pass sees the bits it would have seen.
 * x3d_unscale_sumsq: x3d_grad_sumsq with g[i] = g[i] * (float)state[1] written back in the same pass.  out[0] = the fp64 sum of
 *     squares of the finite UNSCALED entries, out[1] = the number of non-finite ones (inf and nan stay inf and nan); every
 *     `norm` above can be this out[2].  The grid, the scratch layout (x3d_grad_sumsq_scratch(n) doubles) and the fixed
 *     summation order are x3d_grad_sumsq's -- the same walk, instantiated with the product.  Two launches.
 * x3d_seg_unscale_sumsq: the same over a chunk table, with x3d_seg_grad_sumsq's walk and reduction (partials: 2 * nchunk
 *     doubles).  Only elements inside the table's chunks are read or written: a frozen tensor's gradient and the padding keep
 *     their bits and are in neither the sum nor the count.  Two launches.
 *   Because S is a power of two, wherever no product falls below the smallest normal fp32:
 *     S = 1:   g keeps its bits and out has the bits of x3d_grad_sumsq / x3d_seg_grad_sumsq over g.
 *     S = 2^k: g becomes exactly g * 2^-k, and out[0] * S^2 equals, bit for bit, the out[0] of x3d_grad_sumsq /
 *              x3d_seg_grad_sumsq over the scaled gradient; out[1] is the same count.
 * x3d_loss_scale_update: one workgroup.  Keras' DynamicLossScale from norm = the out[2] the step's update launches have read:
 *     norm[1] != 0: S = max(S / 2, 1), [2] = 0, [3] += 1, [5] = 1
 *     norm[1] == 0: [4] += 1, [2] += 1, [5] = 0; then if [2] >= growth_steps and (float)(2 S) is finite: S = 2 S, [2] = 0
 *     and [1] = 1 / S.
 * Refused before any launch (X3D_ERR_INVALID): a null pointer, n <= 0, growth_steps < 1, a float pointer that is not 4-byte or
 * a double pointer that is not 8-byte aligned, and what x3d_seg_grad_sumsq refuses of a table.
 * ------------------------------------------------------------------------------------------ */
#define X3D_LOSS_SCALE_STATE 8
int x3d_loss_scale_apply(float* x, long long n, const double* state, void* stream);
int x3d_unscale_sumsq(float* g, long long n, const double* state, double* scratch, double* out, void* stream);
int x3d_seg_unscale_sumsq(float* g, const int* chunks, int nchunk, const int* segs, int nseg, const double* state,
                          double* partials, double* out, void* stream);
int x3d_loss_scale_update(double* state, const double* norm, long long growth_steps, void* stream);
/* sum of squares of the masked entries (L2 regularisation loss term), out [1] double += */
int x3d_l2_sumsq(const float* w, const unsigned char* l2_mask, double* out, long long n, void* stream);

/* layout helpers at the module boundary: NTHWC (reference, model.py:113) <-> NCTHW (internal) */
int x3d_nthwc_to_ncthw(const void* src, int src_dtype, void* dst, int dst_dtype, int N, int C,
                       long long P, void* stream);

/* ------------------------------------------------------------------------------------------
 * eval-side view construction: decoded video -> the views x crops clips eval.py feeds the model
 *     reference transforms.py:48-65 (temporal looping sampler), :112-147 (short side -> `size`, bilinear, cast
 *     back to uint8), :149-190 (uniform crop, ceil offsets), utils.py:42-72 (x/255 - mean, / std),
 *     dataloader.py:107-116 (clip order: crops major, then views).
 *     video [F][H][W][3] uint8 (device) -> out [crops*views][T][size][size][3] (X3D_F32 / X3D_BF16), channels-last
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const unsigned char* video;
  void* out;
  int F, H, W;
  int T, views, crops, size;
  float mean[3];
  float std[3];
  int dtype;
} x3d_eval_views_args;
int x3d_eval_views(const x3d_eval_views_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * train-side clip construction (the device half of the training input pipeline; decoding stays on
 * the host): decoded video -> one augmented training clip.
 *     reference transforms.py:31-47 (random start, every `rate`-th frame, the video looped), :112-147
 *     (random_short_side_resize: short side -> int(jitter), long side floor((long/short) * jitter) in float32,
 *     bilinear, cast back to uint8), :199-203 (tf.image.random_crop: one (y0, x0) for every frame of the clip),
 *     :205-206 (flip_left_right on EVERY training clip: `random_hflip` is just `is_training`, dataloader.py:136),
 *     utils.py:42-72 (x/255 - mean, / std).
 *     The random draws (start, jitter, y0, x0) are the caller's: TF's generator streams are not reproduced [TF-3p].
 *     video [F][H][W][3] uint8 (device) -> out [T][size][size][3] (X3D_F32 / X3D_BF16), channels-last
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const unsigned char* video;
  void* out;
  int F, H, W;
  int T, rate, start;          /* frame j of the clip = (start + j * rate) mod F */
  float jitter;                /* short-side target, uniform in [TRAIN_JITTER_SCALES) */
  int size, y0, x0;            /* crop size and offsets inside the resized frame */
  int flip;                    /* 1: mirror left-right (the reference always does in training) */
  float mean[3];
  float std[3];
  int dtype;
} x3d_train_clip_args;
int x3d_train_clip(const x3d_train_clip_args* a, void* stream);
/* extents of a H x W frame after random_short_side_resize with target `jitter` (transforms.py:126-141) */
int x3d_train_resized_hw(int H, int W, float jitter, int* new_h, int* new_w);

/* ------------------------------------------------------------------------------------------
 * batched training augmentation (ABI 138; AUG.* of the config, x3d_tf_amd/aug.py): N decoded videos of DIFFERENT extents ->
 * the whole clip batch out [N][T][size][size][3] (X3D_F32 / X3D_BF16 / X3D_F16, channels-last) in ONE launch, or two when
 * a clip's contrast needs the mean of its geometric output.  The stages and where their definitions come from:
 *     geometry  "jitter" rows: x3d_train_clip's (reference transforms.py:31-47, 112-147, 199-206), bit for bit;
 *               "rrc" rows: torchvision RandomResizedCrop [TV-3p] -- the box [ry0, ry0+rh) x [rx0, rx0+rw) of the source
 *               frame resampled to size x size with half-pixel-centre bilinear weights, no antialias, taps clamped to the
 *               box (torch.nn.functional.interpolate(mode="bilinear", align_corners=False) on the crop), fp32, NOT
 *               truncated to uint8;  frame j = (start + j * rate) mod F;  the mirror is applied last.
 *     colour    PySlowFast color_jitter + grayscale [PSF-3p] on the 0-255 scale, never clamped, hence affine per pixel:
 *               v_c = sum_k M[c][k] * x_k + K * m, m = mean over the T*size*size pixels of the clip's geometric output of
 *               0.299 R + 0.587 G + 0.114 B (aug.fold_color folds the drawn chain into M and K).
 *     normalise (v / 255 - mean) / std   (utils.py:42-72)
 *     erase     timm RandomErasing [TIMM-3p]: the box [ey0, ey1) x [ex0, ex1) of the OUTPUT crop, the same in all T frames,
 *               becomes 0 (X3D_AUG_ERASE_CONST) or N(0, 1) noise (X3D_AUG_ERASE_PIXEL): Philox4x32-10 (Salmon et al., SC'11)
 *               with key = the CLIP'S OWN 64-bit seed (columns SEED_LO, SEED_HI of its row), counter = (pixel index in the
 *               clip lo, hi, clip index, 0), Box-Muller on 24-bit uniforms of the four output words -> one normal per
 *               channel.  Stateless: the same (seed, clip index, element) gives the same value on every run, whatever the
 *               other clips of the batch are.
 *     One round-to-nearest-even to the storage type.  All arithmetic fp32 without contraction.
 * Per-clip parameters are rows of plain tables (no struct): videos [N] device addresses of the uint8 videos [F][H][W][3];
 * geom int32 [N][X3D_AUG_GEOM_COLS]; color fp32 [N][X3D_AUG_COLOR_COLS] = M row-major, then K.  geom and color are DEVICE
 * copies (read by the kernels) of host_geom and host_color (HOST, read by this call: validation, and whether any clip has
 * K != 0).  THE CALLER MUST UPLOAD EXACTLY host_geom AND host_color: the call copies nothing (it neither allocates nor
 * synchronises), so it validates the host rows and cannot see the device rows.  The kernels clamp every tap to the H x W
 * the device row states, take the frame index modulo max(F, 1) and treat a crop extent below 1 as 1, so a device row that
 * differs gives a wrong picture but no division by zero; only F, H, W larger than the allocation read outside it, exactly
 * as a wrong x3d_train_clip_args does.  mean, std: HOST float[3].  scratch: x3d_train_clips_aug_scratch(N, T, size) bytes of device memory, 8-byte
 * aligned, the caller's; it need not be zeroed.
 * The mean pass (only when some K != 0; clips with K == 0 skip it): X3D_AUG_MEAN_PARTS workgroups per clip each write ONE
 * fp64 partial sum of their share of the pixels into scratch; the apply pass adds a clip's partials in ascending order.
 * No floating-point atomics: the same inputs give the same bits on every run.
 * Refused before any launch (X3D_ERR_INVALID): a null table / pointer, N <= 0 or N > 65535, non-positive extents, start
 * outside [0, F), an unknown mode / dtype / erase_mode, a "jitter" crop outside its resized frame (or nh, nw < size), an
 * "rrc" box outside its frame or empty, an erase box outside the crop (0 <= ey0 <= ey1 <= size, likewise x; an empty box:
 * no erase), a non-finite colour coefficient.
 * ------------------------------------------------------------------------------------------ */
#define X3D_AUG_CROP_JITTER 0
#define X3D_AUG_CROP_RRC 1
#define X3D_AUG_ERASE_CONST 0
#define X3D_AUG_ERASE_PIXEL 1
#define X3D_AUG_MEAN_PARTS 32
#define X3D_AUG_GEOM_COLS 18
#define X3D_AUG_G_F 0         /* frames, height, width of the clip's video */
#define X3D_AUG_G_H 1
#define X3D_AUG_G_W 2
#define X3D_AUG_G_START 3
#define X3D_AUG_G_MODE 4      /* X3D_AUG_CROP_* */
#define X3D_AUG_G_NH 5        /* jitter: extents after the short-side resize (x3d_train_resized_hw) */
#define X3D_AUG_G_NW 6
#define X3D_AUG_G_Y0 7        /* jitter: crop offset in the resized frame;  rrc: top-left corner of the box */
#define X3D_AUG_G_X0 8
#define X3D_AUG_G_BH 9        /* rrc: box extents */
#define X3D_AUG_G_BW 10
#define X3D_AUG_G_FLIP 11
#define X3D_AUG_G_EY0 12      /* erase box in the output crop, [EY0, EY1) x [EX0, EX1) */
#define X3D_AUG_G_EY1 13
#define X3D_AUG_G_EX0 14
#define X3D_AUG_G_EX1 15
#define X3D_AUG_G_SEED_LO 16  /* the clip's 64-bit noise seed (X3D_AUG_ERASE_PIXEL), low and high word */
#define X3D_AUG_G_SEED_HI 17
#define X3D_AUG_COLOR_COLS 10
#define X3D_AUG_C_K 9         /* coefficient of the mean gray m (columns 0-8: M) */
long long x3d_train_clips_aug_scratch(int N, int T, int size);
int x3d_train_clips_aug(const long long* videos, const int* geom, const float* color, const int* host_geom,
                        const float* host_color, void* out, void* scratch, int N, int T, int rate, int size,
                        const float* mean, const float* std, int erase_mode, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * RandAugment on the uint8 frames (AUG.AA_TYPE of the config, x3d_tf_amd/aug.py draw_randaug; added under ABI 138 without a
 * bump: new symbols only).  N decoded videos of DIFFERENT extents; clip n takes its T sampled frames
 * (start + j * rate) mod F and sends them through `layers` ops, one op per (clip, layer), every frame of a clip with the
 * same op and argument.  Runs BEFORE x3d_train_clips_aug, which then reads the result as a video of F = T frames with
 * start = 0, rate = 1.  The ops (timm rand_augment_transform as PySlowFast applies it to clips; PIL's arithmetic):
 *     INVERT 255 - v;  SOLARIZE v < IARG ? v : 255 - v;  SOLARIZE_ADD v < 128 ? min(255, v + IARG) : v;
 *     POSTERIZE v & ~(2^(8 - IARG) - 1), IARG >= 8: identity;
 *     AUTOCONTRAST per frame and channel, lo / hi = min / max: hi <= lo identity, else
 *         lut[i] = clamp(trunc(i * (255.0 / (hi - lo)) - lo * (255.0 / (hi - lo))), 0, 255) in fp64 (two products, one difference);
 *     EQUALIZE per frame and channel, histogram h: fewer than 2 non-empty bins identity; step = (sum h - last non-empty bin)
 *         / 255 (integer), step == 0 identity; else n = step / 2, for i = 0..255: lut[i] = min(255, n / step), n += h[i];
 *     COLOR / CONTRAST / BRIGHTNESS / SHARPNESS out = d + f * (v - d) with f = FARG: t = fl32(f * fl32(v - d)), r = fl32(d + t)
 *         (no contraction), result 0 if r <= 0, 255 if r >= 255, else trunc(r).  d: COLOR the pixel's
 *         L = (19595 R + 38470 G + 7471 B + 32768) >> 16; BRIGHTNESS 0; CONTRAST the frame's constant
 *         trunc(sum L / (H * W) + 0.5) (exact integer sum, fp64 division); SHARPNESS (sum k v + 6) / 13 (integer) over the
 *         3 x 3 neighbourhood with k = 1 except 5 at the centre, the frame's one-pixel border copied unchanged;
 *     ROTATE / SHEAR_X / SHEAR_Y / TRANSLATE_X / TRANSLATE_Y one inverse affine map, bilinear: the six X3D_RA_X_A..F columns
 *         are SIGNED FIXED POINT WITH 32 FRACTIONAL BITS in int64 (the host builds the matrix in fp64, folds the +0.5 pixel
 *         centres into C and F, rounds to nearest).  Output pixel (x, y): sx = A x + B y + C, sy = D x + E y + F in int64;
 *         outside [0, W) x [0, H): the fill colour; else subtract half a pixel, tap = floor, weight fx, fy = the top 8
 *         fractional bits, taps clamped to the frame,
 *         ((p00 (256 - fx) + p01 fx)(256 - fy) + (p10 (256 - fx) + p11 fx) fy + 32768) >> 16.
 *     COPY the sampled frames unchanged (a clip without an applied op whose video is not already its T frames);
 *     NONE the clip takes no part in the layer (its workgroups return at once; SRC / DST are not read).
 * Tables (plain arrays, no struct; the DEVICE copies are read by the kernels, the HOST copies validated by this call before
 * any launch -- THE CALLER UPLOADS EXACTLY THE HOST TABLES, as for x3d_train_clips_aug):
 *     videos int64 [N]: device addresses of the uint8 videos [F][H][W][3] (device table only);
 *     clips  int32 [N][X3D_RA_CLIP_COLS]: F, H, W, start;
 *     ops    int32 [N][layers][X3D_RA_OP_COLS]: op code, IARG, FARG (the bits of an fp32), 0;
 *     xform  int64 [N][layers][X3D_RA_X_COLS]: A..F, then SRC and DST: byte offsets into `work` of the T x H x W x 3 bytes
 *            the layer reads and writes; SRC = -1 reads the sampled frames straight from the video.  The caller ping-pongs
 *            each clip between two ranges of its own and keeps the ranges of different clips disjoint.
 * work: device, work_bytes bytes, the caller's.  scratch: x3d_randaug_scratch(N, T) bytes of device memory, 8-byte aligned; the
 * call zeroes it itself (hipMemsetAsync on `stream`) before each statistics launch.  fill_r/g/b: the fill colour, 0..255.
 * Launches: per layer one apply launch over the whole batch (grid z = clip, y = frame; a workgroup reads its clip's op from the
 * device table), preceded -- only when some clip's op in that layer is AUTOCONTRAST, EQUALIZE or CONTRAST -- by one
 * statistics launch whose workgroups return at once for every other clip: LDS histograms (or the L sum) per workgroup,
 * flushed with INTEGER atomics (sums commute: the same bits on every run; no floating-point atomics).  A layer in which every
 * clip has NONE launches nothing.  Neither allocates nor synchronises.
 * Refused before any launch (X3D_ERR_INVALID): a null table / pointer, N <= 0 or N > 65535, T, rate, layers <= 0, T > 65535,
 * F, H or W <= 0 (or H, W > 32768), start outside [0, F), an unknown op, a non-finite FARG of the four blend ops, POSTERIZE
 * bits outside [0, 8], a matrix coefficient out of range (|A|, |B|, |D|, |E| >= 2^45, |C|, |F| >= 2^60), SRC < -1, a SRC or DST
 * range outside [0, work_bytes), SRC and DST ranges of one (clip, layer) overlapping, a fill colour outside 0..255.
 * ------------------------------------------------------------------------------------------ */
#define X3D_RA_NONE 0
#define X3D_RA_AUTOCONTRAST 1
#define X3D_RA_EQUALIZE 2
#define X3D_RA_INVERT 3
#define X3D_RA_ROTATE 4
#define X3D_RA_POSTERIZE 5
#define X3D_RA_SOLARIZE 6
#define X3D_RA_SOLARIZE_ADD 7
#define X3D_RA_COLOR 8
#define X3D_RA_CONTRAST 9
#define X3D_RA_BRIGHTNESS 10
#define X3D_RA_SHARPNESS 11
#define X3D_RA_SHEAR_X 12
#define X3D_RA_SHEAR_Y 13
#define X3D_RA_TRANSLATE_X 14
#define X3D_RA_TRANSLATE_Y 15
#define X3D_RA_COPY 16
#define X3D_RA_CLIP_COLS 4    /* F, H, W, start */
#define X3D_RA_OP_COLS 4
#define X3D_RA_O_OP 0
#define X3D_RA_O_IARG 1       /* POSTERIZE bits, SOLARIZE threshold, SOLARIZE_ADD addend */
#define X3D_RA_O_FARG 2       /* the factor of COLOR / CONTRAST / BRIGHTNESS / SHARPNESS: the bits of an fp32 */
#define X3D_RA_X_COLS 8
#define X3D_RA_X_A 0          /* inverse affine map, 32 fractional bits: sx = A x + B y + C, sy = D x + E y + F */
#define X3D_RA_X_SRC 6
#define X3D_RA_X_DST 7
#define X3D_RA_FRAC_BITS 32
#define X3D_RA_STAT_WORDS 772 /* uint32 words of scratch per (clip, frame): 3 x 256 histogram, the L sum (uint64), padding */
long long x3d_randaug_scratch(int N, int T);
int x3d_randaug_clips(const long long* videos, const int* clips, const int* ops, const long long* xform,
                      const int* host_clips, const int* host_ops, const long long* host_xform, void* work,
                      long long work_bytes, void* scratch, int N, int T, int rate, int layers, int fill_r, int fill_g,
                      int fill_b, void* stream);

/* ------------------------------------------------------------------------------------------
 * JPEG frames of the TFRecord input pipeline decoded on the device (reference dataloader.py:80-88:
 * tf.image.decode_jpeg of every frame; create_tfrecords.py:64-65 writes them).
 *     Baseline and extended-sequential Huffman JPEG, 8-bit, grey or YCbCr with luma sampling 1x1 / 2x1 / 2x2 and
 *     chroma 1x1, optional restart intervals, any extents.  Bit-identical to the libjpeg defaults: ISLOW IDCT,
 *     fancy (triangle) chroma upsampling, 16-bit fixed-point YCbCr -> RGB; grey replicated to RGB.
 *     Anything else is reported per image (X3D_JPEG_UNSUPPORTED / X3D_JPEG_MALFORMED) for the caller to decode
 *     on the host.
 * x3d_jpeg_parse (host only, no GPU): reads the headers of n images (host pointers data[i], lengths[i]) into
 *     imgs[i] and lays out one device scratch for all supported images (*scratch_bytes).  The caller then sets
 *     `data_off` / `data_len` (where image i sits in the packed device copy of the bytes) and `out` (NULL: skip).
 * x3d_jpeg_decode: three launches on `stream` (entropy decode, dequantise + IDCT, upsample + colour convert);
 *     writes status[i] (device) per image: X3D_JPEG_OK, the parse status, X3D_JPEG_SKIPPED, or X3D_JPEG_CORRUPT
 *     (that image's slot is then not written).  X3D_JPEG_OK means that out holds what the host decoder makes of
 *     the same bytes, whether they are a legal stream or a damaged one.  X3D_JPEG_CORRUPT is reported for
 *       - an entropy segment that ends before the last MCU, an invalid Huffman code, a restart interval that
 *         is not followed at once by its RSTn;
 *       - a marker among the bytes left over after the last MCU (the host decoder acts on it);
 *       - a block with a dequantised coefficient beyond +-4095, a value between the two IDCT passes beyond
 *         +-16383 or a sample before the level shift outside [-512, 511].  Up to there libjpeg's C and SIMD
 *         IDCTs give the same integers (the range-limit table is the clamp on [-512, 511] and wraps beyond;
 *         the SIMD code works in 16 and 32 bits and saturates); past it the result depends on the libjpeg
 *         build, so the frame is the host's to decode.  No legal stream tried (q1 to q100, 0 / 255 noise
 *         included) is refused; one whose quantisation error alone passed the sample limit would be.
 *     A frame that lacks only its EOI is decoded.  Reads only bytes [data_off + ecs_off, data_off + ecs_end)
 *     and the tables of image i, writes only its scratch range and out[0 .. height * width * 3).
 * ------------------------------------------------------------------------------------------ */
#define X3D_JPEG_OK 0
#define X3D_JPEG_UNSUPPORTED 1   /* valid JPEG outside the device decoder's scope (progressive, arithmetic, 12-bit, CMYK, ...) */
#define X3D_JPEG_MALFORMED 2     /* header that cannot be parsed */
#define X3D_JPEG_CORRUPT 3       /* (device) entropy-coded data ends early, is invalid or decodes to values outside the IDCT range above */
#define X3D_JPEG_SKIPPED 4       /* (device) supported, but `out` was NULL */
typedef struct {
  unsigned char* out;          /* device [height][width][3] uint8 (caller) */
  long long data_off;          /* offset of the image in the packed device bytes (caller) */
  long long coef_off;          /* int16 coefficients in the scratch, bytes (parse) */
  long long plane_off;         /* uint8 component planes in the scratch, bytes (parse) */
  int data_len;                /* bytes of the image (caller) */
  int status;                  /* X3D_JPEG_* (parse) */
  int height, width, ncomp;
  int hs[3], vs[3];            /* sampling factors (1 x 1 for grey) */
  int bw[3], bh[3];            /* component extents in 8x8 blocks */
  int mcux, mcuy;              /* MCUs per row / column */
  int dc_tbl[3], ac_tbl[3];    /* Huffman table of each component */
  int huff_off[8];             /* offset of the 16 code-length counts of DC tables 0-3, AC tables 0-3 (-1: absent) */
  int restart_interval;        /* MCUs per restart interval, 0: none */
  int ecs_off, ecs_end;        /* entropy-coded segment, offsets from the image start */
  unsigned short qt[3][64];    /* quantisation table of each component, natural order */
} x3d_jpeg_image;
typedef struct {
  const unsigned char* data;             /* the packed bytes of all images */
  const x3d_jpeg_image* images;          /* device copy of the descriptors */
  const x3d_jpeg_image* host_images;     /* host: the same descriptors (launch extents, validation) */
  int n;
  void* scratch;
  long long scratch_bytes;
  int* status;                           /* [n] */
} x3d_jpeg_decode_args;
int x3d_jpeg_parse(const unsigned char* const* data, const int* lengths, int n, x3d_jpeg_image* imgs,
                   long long* scratch_bytes);
int x3d_jpeg_decode(const x3d_jpeg_decode_args* a, void* stream);

/* ------------------------------------------------------------------------------------------
 * host helper: CRC32C (Castagnoli), the checksum of TF tensor-bundle checkpoints
 *     (reference train.py:151-158 / utils.py restore path reads such files through tf.train.Checkpoint)
 * ------------------------------------------------------------------------------------------ */
uint32_t x3d_crc32c(const void* data, size_t n, uint32_t crc);

#ifdef __cplusplus
}
#endif
#endif /* X3D_HIP_H */
