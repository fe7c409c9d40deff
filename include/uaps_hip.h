/* uaps_hip.h -- C ABI of libuaps_hip.so, the MI355X (gfx950) kernels of the UAPS training step.
 *
 * The reference (djene-mengistu/UAPS) is pure Python on PyTorch and has no FFI of its own
 * (SURVEY.md section 8b); each entry point below replaces a chain of PyTorch ops of the reference
 * step, cited as file:line relative to the reference root.  The host side (the uaps_amd Python package) binds
 * these with ctypes; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all memory;
 *   - tensors are dense fp32 NCHW exactly as the reference's decoders produce them; labels and
 *     pseudo-labels are int64 [B,H,W] as torch.argmax / the reference's data loader produce them;
 *   - `stream` is a hipStream_t (0 = the null stream); calls only enqueue work, never synchronise, never allocate, read no
 *     environment variable and are safe under hipGraph capture.  The library keeps exactly this state, all of it set by the
 *     caller through the entry points named here and none of it stream-ordered (change it between steps):
 *       process-wide   the convolution arithmetic (uaps_conv_set_mode) and planner switches (uaps_conv_set_tuning), the pointer
 *                      to the device-resident step state (uaps_set_step_state: NULL outside a state-mode step; two trainers in
 *                      one process each bracket their steps with set / clear, see uaps_amd/graph.py) and, per device, the pointer
 *                      to that device's sticky error word (uaps_set_error_word);
 *       per thread     LEGACY: the one-shot side arguments of the NEXT call (uaps_next_call_hints), consumed and cleared by that call.
 *                      Every entry point that reads them also exists as `<name>_h(const uaps_call_hints* hints, same arguments)`
 *                      (round 6, ABI 3): the hints of THAT call as its first argument (NULL = none), nothing thread-local read or
 *                      written -- safe from any thread, e.g. PyTorch's autograd thread.  The Python package calls only the *_h forms
 *                      and uaps_conv_ex.  (uaps_next_launch_events, a measurement aid of bench.py, stays per thread.)
 *   - return value: 0 on success, a negative UAPS_E* code for bad arguments, a positive hipError_t
 *     if a launch failed.  Nothing throws.
 *   - number of heads D in [1,8] (main + auxiliary decoders), classes C in [2,8].
 */
#ifndef UAPS_HIP_H
#define UAPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* uaps_stream_t; /* hipStream_t */

#define UAPS_MAX_HEADS 8
#define UAPS_MAX_CLASSES 8

#define UAPS_OK 0
#define UAPS_EINVAL (-1)     /* null pointer, non-positive dimension                       */
#define UAPS_ERANGE (-2)     /* D, C, kernel size, dilation or alignment outside what is built */
#define UAPS_EWORKSPACE (-3) /* workspace smaller than uaps_loss_workspace_bytes() reports */
#define UAPS_ENOFORM (-4)    /* a hint that changes what the call computes (uaps_call_hints::dyt_*) has no form in the kernel this
                              * layer runs on: nothing was launched, nothing is wrong with the arguments -- do the work the hint
                              * stood for yourself (uaps_bn_act_bwd_apply) and call again without it.  (Until round 5 this case
                              * shared UAPS_ERANGE with real range errors.) */

int uaps_abi_version(void);
const char* uaps_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * Loss block of the step: UAPS_train.py:186-282 (+ utilities/pytorch_losses.py:54-89 dice_loss,
 * torch.nn.CrossEntropyLoss / KLDivLoss / LogSoftmax objects created at UAPS_train.py:73-75).
 * ------------------------------------------------------------------------------------------- */

/* Layout of the `scalars` output of the two forward calls (float, device).  Offsets in floats. */
/* unsupervised: */
#define UAPS_U_CE(D, C) 0                                   /* ce[D]    CE_k vs pseudo-label (mean)       :259 */
#define UAPS_U_DICE(D, C) (D)                               /* dice[D]  dice_loss_k vs pseudo-label       :259 */
#define UAPS_U_S(D, C) (2 * (D))                            /* s[D]     0.5 (ce+dice)                      :259 */
#define UAPS_U_E(D, C) (3 * (D))                            /* E[D]     mean_pix exp(-var_k)               :265 */
#define UAPS_U_PS(D, C) (4 * (D))                           /* ps_loss                                     :277 */
#define UAPS_U_LUN(D, C) (4 * (D) + 1)                      /* l_uncert                                    :243 */
#define UAPS_U_LOSS(D, C) (4 * (D) + 2)                     /* cw1*ps_loss + cw2*l_uncert                  :282 */
#define UAPS_U_TOTAL(D, C) (4 * (D) + 3)                    /* uaps_pairloss_fwd / _finalize_sums only (round 6): supervised_loss + the
                                                             * slot above = the step's loss (:282), so that the host needs no add launch */
#define UAPS_U_A1(D, C) (4 * (D) + 4)                       /* a1[D*C] = -(2/C)/(card+eps)   (for backward) */
#define UAPS_U_A2(D, C) (4 * (D) + 4 + (D) * (C))           /* a2[D*C] = (2/C) I/(card+eps)^2               */
#define UAPS_U_I(D, C) (4 * (D) + 4 + 2 * (D) * (C))        /* I[D*C]    sum p_kc [y=c]    pytorch_losses.py:85 */
#define UAPS_U_CARD(D, C) (4 * (D) + 4 + 3 * (D) * (C))     /* card[D*C] sum p_kc + [y=c]  pytorch_losses.py:86 */
#define UAPS_U_CNT(D, C) (4 * (D) + 4 + 4 * (D) * (C))      /* cnt[C]    pixels per pseudo-label class      */
#define UAPS_U_NSCALARS(D, C) (4 * (D) + 4 + 4 * (D) * (C) + (C))
/* supervised: */
#define UAPS_S_CE(D, C) 0                                   /* ce[D]                              :194-197 */
#define UAPS_S_DICE(D, C) (D)                               /* dice[D]                            :201-204 */
#define UAPS_S_SUP(D, C) (2 * (D))                          /* sum_k ce_coef*ce_k + dice_coef*dice_k  :218 */
#define UAPS_S_BAD(D, C) (2 * (D) + 1)                      /* number of labels outside [0,C) (must be 0)  */
#define UAPS_S_A1(D, C) (2 * (D) + 2)
#define UAPS_S_A2(D, C) (2 * (D) + 2 + (D) * (C))
#define UAPS_S_I(D, C) (2 * (D) + 2 + 2 * (D) * (C))
#define UAPS_S_CARD(D, C) (2 * (D) + 2 + 3 * (D) * (C))
#define UAPS_S_CNT(D, C) (2 * (D) + 2 + 4 * (D) * (C))
#define UAPS_S_NSCALARS(D, C) (2 * (D) + 2 + 4 * (D) * (C) + (C))

/* Bytes of scratch the forward calls need (block partial sums); same query serves both. */
int uaps_loss_workspace_bytes(int D, int B, int C, int H, int W, size_t* out_host);

/* Unsupervised branch, forward.  Replaces UAPS_train.py:186-189 (softmax), 223 (mean prediction),
 * 226-236 (KL "variance" maps, exp(-var)), 241-243 (l_uncert), 251-255 (Dirichlet-mixed arg-max
 * pseudo-label; w_host are the np.random.dirichlet weights, applied as fp32 scalars left to right),
 * 259-277 (CE + Dice pseudo-supervision weighted by mean(exp(-var))) and the cw-weighted sum of 282.
 *   logits_host : host array of D device pointers, each fp32 [B,C,H,W] contiguous
 *   pseudo      : out int64 [B,H,W]
 *   var         : out fp32 [D,B,H,W] (var_k = sum_c KL(mean || p_k)); may be NULL to skip the store
 *   scalars     : out fp32 [UAPS_U_NSCALARS(D,C)]
 */
int uaps_unsup_fwd(const float* const* logits_host, const double* w_host, int D, int B, int C, int H, int W,
                   float cw1, float cw2, float eps, int64_t* pseudo, float* var, float* scalars,
                   void* workspace, size_t workspace_bytes, uaps_stream_t stream);

/* Unsupervised branch, backward: d(gscale * (cw1*ps_loss + cw2*l_uncert)) / d logits_k, the closed
 * form of what autograd derives from UAPS_train.py:223-282.
 *   gscale  : device pointer to the upstream gradient (one float), or NULL for 1
 *   dlogits_host : host array of D device pointers, each fp32 [B,C,H,W], overwritten
 */
int uaps_unsup_bwd(const float* const* logits_host, const int64_t* pseudo, const float* scalars, float cw1,
                   float cw2, const float* gscale, int D, int B, int C, int H, int W,
                   float* const* dlogits_host, uaps_stream_t stream);

/* Supervised branch: UAPS_train.py:194-218.  loss = sum_k (ce_coef * CrossEntropy_k + dice_coef * dice_loss_k);
 * the reference's supervised_loss (mean over heads of 0.5 (CE + Dice)) is ce_coef = dice_coef = 0.5 / D.
 * With D = 1: (1, 0) is nn.CrossEntropyLoss()(logits, labels) (UAPS_train.py:75) and (0, 1) is
 * dice_loss(labels.unsqueeze(1), logits, eps) (utilities/pytorch_losses.py:54-89). */
int uaps_sup_fwd(const float* const* logits_host, const int64_t* labels, int D, int B, int C, int H, int W,
                 float ce_coef, float dice_coef, float eps, float* scalars, void* workspace,
                 size_t workspace_bytes, uaps_stream_t stream);
int uaps_sup_bwd(const float* const* logits_host, const int64_t* labels, const float* scalars, float ce_coef,
                 float dice_coef, const float* gscale, int D, int B, int C, int H, int W,
                 float* const* dlogits_host, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Step state for captured steps (hipGraph replay freezes kernel arguments).  A 64-byte device buffer the host refreshes
 * before every step: words 0-1 a uint64 added to every Philox key (new draws per step), words 2-9 the mixing weights
 * w[8] as float (UAPS_train.py:251), word 10 / 11 cw1 / cw2 (:279-280), word 12 / 13 Adam's lr / (1 - beta1^t) and
 * 1 / sqrt(1 - beta2^t).  With a state set, uaps_pairloss_fwd accepts w_host = NULL, uaps_pairloss_* read cw1 / cw2 from it
 * when passed NaN, uaps_adam_step reads its two scalars from it when step < 1, the perturbation / dropout kernels add the
 * key increment, and uaps_fanout_perturbed draws a FeatureDropout threshold factor on the device for every u[g] < 0.
 * Process-wide (not per stream); NULL (the default) restores the by-value behaviour.
 * ------------------------------------------------------------------------------------------- */
int uaps_set_step_state(const void* device_ptr);
const void* uaps_get_step_state(void);

/* ---------------------------------------------------------------------------------------------
 * General strided convolutions and the stem max-pool of the reference's ResNet (utilities/resnet.py:120 conv 7x7 / 2 pad 3,
 * :124 max-pool 3x3 / 2 pad 1, :8-14 + :147 layer2's 3x3 / 2 and 1x1 / 2): odd kernel sizes <= 7, stride 1 or 2, bias-free,
 * fp32 NCHW, on the exact-f32 matrix instruction (csrc/conv_strided.hip).  They replace aten::convolution(_backward) and
 * aten::max_pool2d_with_indices(_backward) for those layers.  Packed weights: wf [ks*ks][Cin4][Cout16], wb [ks*ks][Cout4][Cin16]
 * (sizes in floats from uaps_convs_pack_floats).  Output size: OH = (H + 2 pad - ks) / stride + 1.
 * Weight gradient: ks 1, 3, 7 (UAPS_ERANGE otherwise).  A 7x7 / 2 / 3 layer of <= 3 input channels whose OW % 4 == 0 runs the stem
 * form when dy is 16-byte aligned and the general form otherwise; uaps_convs_wrw_workspace_bytes cannot see dy and reports the
 * larger of the two needs, uaps_convs_bwd_weight checks workspace_bytes against the form it runs (UAPS_EWORKSPACE).
 * ------------------------------------------------------------------------------------------- */
int uaps_convs_pack_floats(int Cout, int Cin, int ks, size_t* fwd_floats_host, size_t* bwd_floats_host);
int uaps_convs_pack_weights(const float* w, int Cout, int Cin, int ks, float* wf, float* wb, uaps_stream_t stream);
int uaps_convs_out_size(int H, int W, int ks, int stride, int pad, int* OH_host, int* OW_host);
int uaps_convs_fwd(const float* x, const float* wf, float* y, int B, int Cin, int Cout, int H, int W, int ks, int stride, int pad,
                   uaps_stream_t stream);
int uaps_convs_bwd_data(const float* dy, const float* wb, float* dx, int B, int Cin, int Cout, int H, int W, int ks, int stride,
                        int pad, uaps_stream_t stream);
int uaps_convs_wrw_workspace_bytes(int B, int Cin, int Cout, int H, int W, int ks, int stride, int pad, size_t* bytes_host);
int uaps_convs_bwd_weight(const float* dy, const float* x, float* dw, int B, int Cin, int Cout, int H, int W, int ks, int stride,
                          int pad, void* workspace, size_t workspace_bytes, uaps_stream_t stream);
/* planes = B*C; y [planes, OH, OW] with OH = (H - 1) / 2 + 1; idx: uint8 [planes, OH, OW], the window position of each arg-max
 * (first maximum wins, a NaN replaces whatever is held, so of several NaNs the last: torch.nn.MaxPool2d(3, 2, 1)) */
int uaps_maxpool3x3s2_fwd(const float* x, float* y, void* idx, long planes, int H, int W, uaps_stream_t stream);
int uaps_maxpool3x3s2_bwd(const float* dy, const void* idx, float* dx, long planes, int H, int W, uaps_stream_t stream);
/* y [planes, OH, OW] = x[:, ::2, ::2] (OH = (H - 1) / 2 + 1) and its adjoint (dx [planes, H, W]: dy at the even positions, zero
 * elsewhere): the sampling of a 1x1 / stride 2 convolution (utilities/resnet.py:13-14, 157-161), which then runs as a
 * stride-1 uaps_conv_fwd on the sampled tensor */
/* inverse == 0: xs [B, 4, C, H/2, W/2] = the four stride-2 sampling phases of x [B, C, H, W] (xs[b][2 py + px][c][i][j] =
 * x[b][c][2 i + py][2 j + px]); inverse != 0: the first pointer is xs, the second receives x.  H % 2 == 0, W % 8 == 0, 16-byte
 * aligned pointers (UAPS_ERANGE otherwise).  A 3x3 / stride 2 / padding 1 convolution (utilities/resnet.py:8-10 with stride 2)
 * is a stride-1 uaps_conv_fwd over xs with re-arranged weights */
int uaps_space_to_depth2(const float* x, float* xs, int B, int C, int H, int W, int inverse, uaps_stream_t stream);
int uaps_subsample2_fwd(const float* x, float* y, long planes, int H, int W, uaps_stream_t stream);
int uaps_subsample2_bwd(const float* dy, float* dx, long planes, int H, int W, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The whole loss block of one training step -- UAPS_train.py:194-218 on the labelled logits and :186-189, 223-282 on the
 * unlabelled logits -- as ONE forward launch (+ a one-block finalize) and ONE backward launch: the first blocks of the
 * grid run the supervised branch, the rest the unsupervised branch.  Against uaps_sup_* + uaps_unsup_*: the pseudo-labels
 * are bit-identical, the variance maps agree to a few ulp (the instantiations contract their multiply-adds differently), and the
 * reduced scalars and the gradients that depend on them agree to fp32 summation-order accuracy -- the persistent blocks
 * partition the pixels differently (tests/test_gpu_pairloss.py, tests/test_gpu_loss_forms.py).  Every launch is bitwise
 * reproducible run to run, and the backward writes the same gradient bits with and without uaps_call_hints::out_amax.
 * lab_logits / un_logits: D host pointers
 * each, [B,C,H,W] fp32; ce_coef = dice_coef = 0.5 / D (UAPS_train.py:208-218).  `cfg` = 0, or a cap on the blocks per branch.
 *
 * Gathered-batch semantics.  The reference's nn.DataParallel (UAPS_model.py:13) gathers the logits of all GPUs and computes
 * every CE mean, Dice sum and uncertainty mean over that global batch (UAPS_train.py:194-277).  One process per GPU
 * reproduces it with a 1-step exchange: pass `sums_out` (device, uaps_pairloss_num_sums doubles) to uaps_pairloss_fwd -- it
 * then writes this rank's raw sums and no scalars --, sum the buffers over the ranks (one tiny all-reduce), call
 * uaps_pairloss_finalize_sums with the global pixel count, and give that count to uaps_pairloss_bwd as `n_pixels_loss`
 * (0 = the local B*H*W).  The parameter gradients of the ranks then ADD up to the gradient of the global loss.
 * ------------------------------------------------------------------------------------------- */
int uaps_pairloss_workspace_bytes(int D, int C, size_t* bytes_host);
int uaps_pairloss_num_sums(int D, int C, int* count_host);
int uaps_pairloss_fwd(const float* const* lab_logits_host, const float* const* un_logits_host, const int64_t* labels,
                      const double* w_host, int D, int B, int C, int H, int W, float cw1, float cw2, float eps,
                      int64_t* pseudo, float* var /* [D,B,H,W] or NULL */, float* sup_scalars, float* unsup_scalars,
                      double* sums_out /* NULL: finalise locally */, void* workspace, size_t workspace_bytes, int cfg,
                      uaps_stream_t stream);
int uaps_pairloss_finalize_sums(const double* sums, int D, int C, long n_pixels, float cw1, float cw2, float eps,
                                float* sup_scalars, float* unsup_scalars, uaps_stream_t stream);
int uaps_pairloss_bwd(const float* const* lab_logits_host, const float* const* un_logits_host, const int64_t* labels,
                      const int64_t* pseudo, const float* sup_scalars, const float* unsup_scalars, float cw1, float cw2,
                      const float* gscale, int D, int B, int C, int H, int W, long n_pixels_loss,
                      float* const* dlab_host, float* const* dun_host, int cfg, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Feature perturbations of the auxiliary decoders: utilities/UAPS_unet.py:156-185, applied to all
 * five encoder scales at UAPS_unet.py:227-231.  Random numbers: Philox4x32-10 keyed by `seed`,
 * counter = element index + `offset` (the reference draws from the unseeded CPU generators, so
 * bit parity of the draws is impossible; the *_apply forms take recorded draws for parity tests).
 * ------------------------------------------------------------------------------------------- */

/* FeatureNoise (UAPS_unet.py:172-185): y = x*n + x, n ~ U(-range, range) of shape [C,H,W] shared by
 * the batch.  Backward = the same call on dy with the same seed.  noise_out (fp32 [C,H,W]) may be NULL. */
int uaps_feat_noise(const float* x, float* y, int B, int C, int H, int W, uint64_t seed, uint64_t offset,
                    float range, float* noise_out, uaps_stream_t stream);
/* Same with a given noise tensor (fp32 [C*H*W]); chw = C*H*W. */
int uaps_feat_noise_apply(const float* x, const float* noise, float* y, int B, long chw, uaps_stream_t stream);

/* Dropout(x, p) = F.dropout(x, p, training=True) (UAPS_unet.py:156-158): y = x * keep / (1-p).
 * Backward = the same call on dy with the same seed.  keep_out (uint8 [n]) may be NULL. */
int uaps_feat_bernoulli(const float* x, float* y, long n, uint64_t seed, uint64_t offset, float p,
                        uint8_t* keep_out, uaps_stream_t stream);
int uaps_feat_mask_apply(const float* x, const uint8_t* keep, float scale, float* y, long n, uaps_stream_t stream);

/* FeatureDropout (UAPS_unet.py:161-169): y = x * (mean_c x < u * max_hw mean_c x), u = the
 * np.random.uniform(0.7, 0.9) draw.  keep [B,H,W] uint8 is written for the backward (dx = dy * keep).
 * workspace: uaps_feat_dropout_workspace_bytes() bytes, 16-byte aligned -- the attention map inside it is read and written 16
 * bytes at a time; uaps_feat_dropout_fwd, uaps_feat_dropout_stats and uaps_fanout_perturbed refuse any other workspace with
 * UAPS_EINVAL and write nothing.  A pixel is kept when its attention is strictly below fl(max * u): a pixel at the threshold is
 * dropped, an image whose attention is negative everywhere keeps every pixel, an all-zero image drops every pixel. */
int uaps_feat_dropout_workspace_bytes(int B, int C, int H, int W, size_t* out_host);
int uaps_feat_dropout_fwd(const float* x, float* y, int B, int C, int H, int W, float u, uint8_t* keep,
                          void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_feat_dropout_bwd(const float* dy, const uint8_t* keep, float* dx, int B, int C, int H, int W,
                          uaps_stream_t stream);

/* Gradient fan-in of an encoder feature map that feeds several decoders (UAPS_unet.py:226-232 use each
 * feature list once per decoder): out = in[0] + ... + in[n-1], left to right, n in [1,4], `count` floats. */
int uaps_sum_tensors(const float* const* in_host, int n, float* out, long count, uaps_stream_t stream);
/* The same fan-in with the backward of the perturbations folded in: out = sum_k P_k(g_k), where P_k re-applies the
 * perturbation in front of decoder k to its incoming gradient (all three are diagonal, so backward = forward on the
 * gradient): mode 0 identity (main decoder), 1 FeatureNoise (Philox offsets per statistics group, `range`),
 * 2 Dropout (one offset, `p`), 3 FeatureDropout (keep mask uint8 [B,H,W] from the forward), 4 the MaxPool2d(2) that
 * feeds the next encoder level (g is [B,C,H/2,W/2], keep = the arg-max positions of uaps_maxpool2x2_fwd).  Host arrays of n <= 8
 * entries; offsets is [n][groups]; groups <= 4; needs H*W % 4 == 0 and 16-byte aligned tensors. */
int uaps_fanin_perturbed(const float* const* g_host, const int* mode_host, const uint8_t* const* keep_host,
                         const uint64_t* offsets_host, int n, int groups, uint64_t seed, float range, float p, int B,
                         int C, int H, int W, float* out, uaps_stream_t stream);

/* The forward counterpart: the n perturbed copies of a feature map (UAPS_unet.py:227-231) written by one pass over f
 * instead of one kernel (and one read of f) per perturbation, with the stand-alone kernels' arithmetic and Philox
 * indexing.  mode 1 FeatureNoise, 2 Dropout, 3 FeatureDropout: run uaps_feat_dropout_stats(f, ...) first (channel-mean
 * attention map + per-image maximum into the uaps_feat_dropout_workspace_bytes(B, ...) workspace) and pass that workspace
 * and the threshold factors u [groups]; keep_host[k] receives the uint8 [B,H,W] mask of a mode-3 output.
 * Host arrays of n <= 8 entries, offsets [n][groups], groups <= 4, H*W % 4 == 0, 16-byte aligned tensors. */
int uaps_feat_dropout_stats(const float* x, int B, int C, int H, int W, void* workspace, size_t workspace_bytes,
                            uaps_stream_t stream);
int uaps_fanout_perturbed(const float* f, float* const* out_host, const int* mode_host, uint8_t* const* keep_host,
                          const uint64_t* offsets_host, const float* u_host, const void* fdrop_workspace, int n, int groups,
                          uint64_t seed, float range, float p, int B, int C, int H, int W, uaps_stream_t stream);

/* nn.MaxPool2d(2) of DownBlock (UAPS_unet.py:55-58): out [B,C,H/2,W/2] plus the arg-max position (dy*2+dx) per output
 * as uint8 (first maximum wins, NaN propagates).  Needs H even, W % 8 == 0, 16-byte aligned x/out.  Its backward is
 * mode 4 of uaps_fanin_perturbed (no zero fill, no scatter, no separate accumulation). */
int uaps_maxpool2x2_fwd(const float* x, int B, int C, int H, int W, float* out, uint8_t* idx, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ConvBlock / UpBlock glue between the convolutions (utilities/UAPS_unet.py:36-44, 81-86).
 * ------------------------------------------------------------------------------------------- */

/* nn.BatchNorm2d (training statistics) -> nn.LeakyReLU(slope) -> nn.Dropout(drop_p) on a conv
 * output y [B,C,H,W], fused (UAPS_unet.py:38-40, 42-43).  conv_bias (may be NULL) is the bias of the
 * preceding conv when the caller ran the conv without it: train-mode BN cancels it exactly, it only
 * enters running_mean.  Updates running_mean/running_var (momentum form of nn.BatchNorm2d, unbiased
 * variance) and increments *num_batches_tracked when those pointers are non-NULL.  Writes
 * save_mean/save_invstd [C] for the backward.  Dropout keep-masks come from Philox(seed, offset)
 * and are regenerated by the backward; drop_p = 0 disables it. */
int uaps_bn_workspace_bytes(int B, int C, int H, int W, size_t* out_host);
int uaps_bn_act_fwd_train(const float* y, const float* conv_bias, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                          float eps, float slope, float drop_p, uint64_t seed, uint64_t offset, int B, int C,
                          int H, int W, float* out, float* save_mean, float* save_invstd, void* workspace,
                          size_t workspace_bytes, uaps_stream_t stream);
/* The same with `groups` statistics groups: the batch is `groups` consecutive blocks of B/groups images, each
 * normalised with its own batch statistics (save_mean / save_invstd are [groups][C]) and folded into the running
 * statistics one after the other, exactly as `groups` separate calls in order would (the reference runs the
 * labelled and the unlabelled batch as two forwards, UAPS_train.py:177,185); num_batches_tracked += groups.
 * groups in [1,8], B % groups == 0. */
int uaps_bn_act_fwd_train_grouped(const float* y, const float* conv_bias, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                                  float eps, float slope, float drop_p, uint64_t seed, uint64_t offset, int B, int C,
                                  int H, int W, int groups, float* out, float* save_mean, float* save_invstd,
                                  void* workspace, size_t workspace_bytes, uaps_stream_t stream);
/* The same, with the statistics pass already done by the producer of y: `partials` is float2
 * [C][B][parts_per_image] of per-image partial (sum, sum of squares), as uaps_conv_fwd_stats writes them. */
int uaps_bn_act_fwd_train_partials(const void* partials, int parts_per_image, const float* y, const float* conv_bias,
                                   const float* gamma, const float* beta, float* running_mean, float* running_var,
                                   int64_t* num_batches_tracked, float momentum, float eps, float slope, float drop_p,
                                   uint64_t seed, uint64_t offset, int B, int C, int H, int W, int groups, float* out,
                                   float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                                   uaps_stream_t stream);
int uaps_bn_act_bwd_grouped(const float* dout, const float* y, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, float slope, float drop_p, uint64_t seed,
                            uint64_t offset, int B, int C, int H, int W, int groups, float* dy, float* dgamma,
                            float* dbeta, void* workspace, size_t workspace_bytes, uaps_stream_t stream);
/* The same, also writing the gradient of the conv bias in front of the BatchNorm (identically zero: the bias cancels
 * in train-mode normalisation) into dconv_bias [C], which saves the host a fill launch per layer. */
int uaps_bn_act_bwd_grouped_bias(const float* dout, const float* y, const float* gamma, const float* beta,
                                 const float* save_mean, const float* save_invstd, float slope, float drop_p,
                                 uint64_t seed, uint64_t offset, int B, int C, int H, int W, int groups, float* dy,
                                 float* dgamma, float* dbeta, float* dconv_bias, void* workspace, size_t workspace_bytes,
                                 uaps_stream_t stream);
/* eval(): running statistics, no dropout.  save_mean receives running_mean - conv_bias (for the backward). */
int uaps_bn_act_fwd_eval(const float* y, const float* conv_bias, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float eps, float slope, int B,
                         int C, int H, int W, float* out, float* save_mean, void* workspace,
                         size_t workspace_bytes, uaps_stream_t stream);
/* Backward of the train-mode op: dy [B,C,H,W], dgamma [C], dbeta [C] from dout and the saved y. */
int uaps_bn_act_bwd(const float* dout, const float* y, const float* gamma, const float* beta,
                    const float* save_mean, const float* save_invstd, float slope, float drop_p, uint64_t seed,
                    uint64_t offset, int B, int C, int H, int W, float* dy, float* dgamma, float* dbeta,
                    void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_bn_act_bwd_eval(const float* dout, const float* y, const float* gamma, const float* beta,
                         const float* mean_eff, const float* running_var, float eps, float slope, int B, int C,
                         int H, int W, float* dy, void* workspace, size_t workspace_bytes, uaps_stream_t stream);

/* UpBlock.forward lines 83-85: out[:, :Cs] = skip ; out[:, Cs:] = bilinear x2 (align_corners=True) of
 * low [B,Cl,h,w]; out is [B,Cs+Cl,2h,2w].  Backward: dskip = dout[:, :Cs] (may be NULL), dlow = the
 * transposed interpolation of dout[:, Cs:] (gather form, deterministic).  No pointer needs an alignment beyond its
 * element's: a dout, dskip or skip / out that is not 16-byte aligned takes the element-wise loads and stores. */
int uaps_up_cat_fwd(const float* skip, const float* low, float* out, int B, int Cs, int Cl, int h, int w,
                    uaps_stream_t stream);
int uaps_up_cat_bwd(const float* dout, float* dskip, float* dlow, int B, int Cs, int Cl, int h, int w,
                    uaps_stream_t stream);

/* Bound i (out + i * UAPS_BOUND_FLOATS, see uaps_next_call_hints) = max_c(|gamma_i[c]| + |beta_i[c]|) for n BatchNorm layers
 * (host arrays of n device pointers / channel counts; out holds n * UAPS_BOUND_FLOATS floats), one launch: times sqrt(elements per channel and statistics group) this bounds every output of the train-mode
 * BatchNorm (+ LeakyReLU) of utilities/UAPS_unet.py:38-39 (|x_hat| <= sqrt(n - 1) for batch statistics), the operand bound
 * of the convolutions behind it (uaps_next_call_hints). */
int uaps_bn_param_bounds(const float* const* gamma_host, const float* const* beta_host, const int* C_host, int n, float* out,
                         uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Convolutions of the U-Net: every nn.Conv2d of utilities/UAPS_unet.py (ConvBlock 3x3 :36-44,
 * UpBlock.conv1x1 :73, Decoder.out_conv :138-139; stride 1, padding ks/2, ks in {1,3}), fp32 NCHW,
 * computed as an implicit GEMM on the matrix cores in one of three arithmetic modes (uaps_conv_set_mode):
 *   2 (default)  as 1, and where the caller supplies magnitude bounds of the tensor operands (uaps_next_call_hints):
 *                both fp32 operands scaled by a power of two and split into two fp16 pieces (22 significant bits),
 *                three partial products per multiply on v_mfma_f32_*_f16 with fp32 accumulation -- an error below that of
 *                the fp32 matrix instruction's accumulation chain (tests/test_gpu_conv.py) at twice the rate of mode 1,
 *   1            exact three-way bf16 split of both fp32 operands, six partial products per multiply on
 *                v_mfma_f32_16x16x32_bf16 with fp32 accumulation: the error of an fp32 fma chain at 2.67x the
 *                fp32 matrix rate (csrc/conv_split.hpp); used for 16-byte-aligned rows without dilation,
 *   0            the exact-f32 matrix instruction v_mfma_f32_16x16x4_f32 for everything (also: UAPS_CONV_MODE=0,
 *                or bit 28 of `cfg` for one call).
 * They replace the three aten::convolution / convolution_backward calls PyTorch makes per layer.
 *
 * Weights are used in a packed, zero-padded layout produced by uaps_conv_pack_weights from the
 * nn.Conv2d.weight tensor [Cout][Cin][ks][ks]:
 *   wf [ks*ks][Kpad(Cin)][Npad(Cout)]   for the forward,
 *   wb [ks*ks][Kpad(Cout)][Npad(Cin)]   (transposed, taps flipped) for the input gradient,
 * sizes (in floats) from uaps_conv_pack_floats.  `cfg` = 0 selects the tiling automatically; other
 * values are tuning overrides used by tools/bench_conv.py (low byte: output channels per workgroup,
 * 16/32/64; bits 8-9: 1 = 8x32 pixel tile, 2 = 16x16; for bwd_weight the low 24 bits: number of pixel splits).
 * Bits 24-27 of `cfg` are functional: the dilation of a 3x3 kernel, 0/1 (none), 2 or 4, with padding = dilation
 * (the dilated stages of utilities/resnet.py:8-10, 201-203); pass the same value to all three directions.
 * ------------------------------------------------------------------------------------------- */
int uaps_conv_set_mode(int mode);      /* 0 / 1 / 2 as above (default 2); process-wide, not stream-ordered: set it between steps */
/* Planner switches for ablation runs and diagnosis (tools/ablation.sh, tools/diag); 0 = the shipped plan. */
#define UAPS_TUNE_NO_SPLIT_FWD 1u      /* forward / input gradient on the fp32 matrix instruction whatever the mode */
#define UAPS_TUNE_NO_SPLIT_WRW 2u      /* weight gradient likewise */
#define UAPS_TUNE_NO_SMALL 4u          /* no exact-N class kernels (csrc/conv_small.hpp) */
#define UAPS_TUNE_NO_HP16 8u           /* no persistent 16-output-channel kernels (csrc/conv_split_n16.hpp) */
#define UAPS_TUNE_WRW_ROW_MAJOR 16u    /* split weight gradient: row-major instead of column-strip tile order */
#define UAPS_TUNE_WRW_SHORT_TILES 32u  /* split weight gradient: 4-row tiles also on the 16-output-channel layers */
#define UAPS_TUNE_NO_TALL_FWD 64u     /* forward / input gradient of 32-channel blocks: 8-row tiles instead of 16-row ones */
#define UAPS_TUNE_NO_ROW16 128u       /* no full-width-row kernels (csrc/conv_split_row16.hpp): the 8 x 32-tile persistent kernels instead */
#define UAPS_TUNE_NO_ROW_WRW 256u     /* no full-width-row weight-gradient kernels (csrc/conv_split_wrw_row.hpp) */
#define UAPS_TUNE_DEEP_ROWS 512u      /* diagnostic: the full-width-row kernels with two row sets in flight (round 5: measured slower) */
#define UAPS_TUNE_G1_NARROW 1024u    /* 1x1 GEMM kernels: 128 output channels per workgroup also where 256 divide the layer's width */
#define UAPS_TUNE_NO_G 2048u         /* no whole-layer-width tile kernels (csrc/conv_split_g.hpp, round 6): the 8 x 32-tile kernels instead */
#define UAPS_TUNE_G_DEEP 4096u       /* diagnostic: those kernels with all nine taps' weight fragments in registers, loaded around the fetch */
int uaps_conv_set_tuning(unsigned flags);
unsigned uaps_conv_get_tuning(void);

/* Sticky device error word.  The fp16-split convolutions (mode 2) trust the magnitude bounds they are handed: a bound that
 * is too small by more than the 2x headroom lets a scaled operand overflow fp16, and every output it touches comes back
 * NaN.  Those kernels check what they store and OR a UAPS_ERR_* bit into *device_word (4-byte aligned device memory owned
 * and zeroed by the caller; NULL = no reporting) when a stored value is not finite -- so a violated bound, or non-finite data
 * entering a convolution, is reported instead of training on.  Read the word whenever the host synchronises anyway
 * (UAPSTrainer.epoch_metrics / validate / check_errors do).  One word per DEVICE: the call binds (or, with NULL, unbinds) the
 * word of the current device, and a launch reports to the word of the device it runs on.  The word must outlive every
 * launch made while it is bound (the Python package keeps one never-freed word per device, uaps_amd._lib.error_word). */
#define UAPS_ERR_CONV_NONFINITE 1u     /* an fp16-split forward / input-gradient convolution stored a non-finite value */
#define UAPS_ERR_WRW_NONFINITE 2u      /* an fp16-split weight-gradient convolution produced a non-finite partial sum */
int uaps_set_error_word(unsigned* device_word);

/* One-shot side arguments for the NEXT kernel entry point called on this thread; that call consumes and clears them
 * (every convolution entry point, uaps_bn_act_fwd_train_partials, uaps_bn_finalize_train, uaps_bn_act_bwd*,
 * uaps_pairloss_bwd, uaps_up_cat_fwd and uaps_add_relu do; NULL clears).
 *   bound[i], mul[i]  device bound b and host factor m > 0 with |operand i| <= value(b) * m for every element; NULL = unknown.
 *                     A bound is UAPS_BOUND_FLOATS floats (16-byte aligned): value(b) = max over the UAPS_BOUND_SLOTS
 *                     floats b[k * UAPS_BOUND_STRIDE], the rest is padding -- the producing kernels raise the slots with
 *                     atomics, and thousands of workgroups on ONE address would serialise at the memory side.
 *                     Operands: conv forward: 0 = x (for the *_bn entry points: the activation after the fused
 *                     BatchNorm + LeakyReLU), 1 = x2 of *_cat;  conv bwd_data: 0 = dy;  conv bwd_weight: 0 = dy, 1 = x, 2 = x2.
 *                     In mode 2 a 3x3 convolution whose tensor operands all carry a bound runs in the two-piece fp16 form;
 *                     without bounds it runs as in mode 1.  A bound that is too small makes the result wrong (fp16
 *                     overflow), one that is too large by up to 2^10 costs no accuracy.
 *   stats_mean, stats_bias   per-channel device arrays [Cout] (either may be NULL = 0): a convolution that writes BatchNorm
 *                     partial sums (uaps_conv_fwd_stats, the stats output of uaps_conv_fwd_bn / _cat) forms them about the
 *                     shift s_c = stats_mean[c] - stats_bias[c], i.e. sum(v - s), sum((v - s)^2) -- pass the BatchNorm's
 *                     running_mean and the bias of the convolution in front of it, and the variance E[d^2] - E[d]^2 no
 *                     longer cancels for channels with |mean| >> std (fp32 partial sums).  The call that CONSUMES those
 *                     partials (uaps_bn_act_fwd_train_partials, uaps_bn_finalize_train) must be given the same two
 *                     pointers in its own hints; it reads them before it updates running_mean.
 *   out_amax          a bound (UAPS_BOUND_FLOATS floats, zero-initialised by the caller WITH uaps_zero_bounds) whose slots the
 *                     producing kernel raises atomically so that value(out_amax) = maximum |element| of its output tensor: the
 *                     bound of a later convolution's operand.
 * Bound storage is read by the kernels with agent-scope loads and raised by memory-side atomics; whoever else writes it must
 * write past the per-XCD L2s too (uaps_zero_bounds, uaps_bn_param_bounds do; a plain fill or copy of the same kernel stream is
 * coherent only after that kernel has ended -- under a hipGraph replay not even then). */
#define UAPS_BOUND_SLOTS 16
#define UAPS_BOUND_STRIDE 64
#define UAPS_BOUND_FLOATS (UAPS_BOUND_SLOTS * UAPS_BOUND_STRIDE)
typedef struct uaps_call_hints {
    unsigned struct_size;        /* sizeof(uaps_call_hints) of the header the CALLER was built against (round 5).  A shorter struct of
                                  * an older client is accepted and its missing tail reads as zero; 0 or a size beyond this library's
                                  * struct is UAPS_EINVAL -- fields are only ever appended */
    const float* bound[3];
    float mul[3];
    float* out_amax;
    const float* stats_mean;     /* see below */
    const float* stats_bias;
    const float* residual;       /* uaps_bn_act_fwd_train_*: out = relu(bn(y) + residual) -- a residual join (utilities/resnet.py:47-50,
                                  * 88-91) in the BatchNorm's apply pass; slope is ignored, drop_p must be 0; out_amax is honoured */
    /* uaps_conv_bwd_weight_partial*: the `dy` argument is the gradient BEHIND the BatchNorm + LeakyReLU that follows the
     * convolution (d(activation)); the kernel forms dy = BatchNorm backward of it while staging -- from dyt_y (the convolution's
     * raw output), dyt_coef (uaps_bn_act_bwd_prepare) -- and writes it to dyt_out for the input-gradient call.  bound[0] must
     * then be the bound uaps_bn_act_bwd_prepare raised.  UAPS_ENOFORM (nothing launched) when the layer's kernel has no such
     * form: run uaps_bn_act_bwd_apply and call again without these. */
    const float* dyt_y;
    const float* dyt_coef;
    float* dyt_out;
    float dyt_slope;
    int dyt_groups;
    /* uaps_conv_bwd_data (round 5): the input gradient this call produces IS d(activation) of a train-mode BatchNorm + LeakyReLU
     * (the layer in front of the convolution); its kernel also forms that BatchNorm's backward sums -- what the first pass of
     * uaps_bn_act_bwd_prepare computes from (gradient, y) -- in its epilogue: bsum_y the BatchNorm's raw input [B, Cin, H, W],
     * bsum_mean / bsum_invstd [groups][Cin] and bsum_gamma / bsum_beta [Cin] its saved statistics and parameters, bsum_partials
     * float2 [Cin][B][H / 16] (sum d, sum d x_hat per 16-row run of the kernel),
     * bsum_max two zeroed bounds (2 * UAPS_BOUND_FLOATS floats: max|d|, max|x_hat|).  uaps_bn_act_bwd_finalize then replaces
     * uaps_bn_act_bwd_prepare.  UAPS_ENOFORM (nothing launched) where the layer's kernel has no such form (built: the
     * full-width-row kernel, 16 -> 16 channels on a 256-wide map). */
    const float* bsum_y;
    const float* bsum_mean;
    const float* bsum_invstd;
    const float* bsum_gamma;
    const float* bsum_beta;
    void* bsum_partials;
    float* bsum_max;
    float bsum_slope;
    int bsum_groups;
} uaps_call_hints;
int uaps_next_call_hints(const uaps_call_hints* hints);
/* Measurement aid (bench.py): `start` / `stop` are two hipEvent_t created with timing enabled.  The calling thread's next MAIN
 * kernel launch -- the convolution kernel of uaps_conv_fwd* / uaps_conv_bwd_data* / uaps_conv_bwd_weight* / uaps_convs_*, the
 * forward / backward kernel of uaps_pairloss_fwd / _bwd; not their packing, reduce or finalize launches -- attaches them to its
 * dispatch (hipExtLaunchKernel), so that hipEventElapsedTime(start, stop) is that kernel's execution time as a profiler's kernel
 * trace reports it.  One-shot; (NULL, NULL) disarms.  Returns 1 when the previously armed pair was consumed by a launch since
 * the last call, else 0. */
int uaps_next_launch_events(void* start, void* stop);
/* Measurement aid (bench.py: roofline.step_algorithmic_bytes).  uaps_account(1) zeroes a process-wide tally and switches it on:
 * from then on every kernel entry point of this library adds the ALGORITHMIC bytes of the launch it enqueues -- every operand
 * tensor read once and every result written once, fp32 / int64 as the reference holds them (SURVEY.md 8d's per-unit figures);
 * workspaces, partial sums, halo and packed-weight re-reads are not counted.  uaps_account(0) stops counting;
 * uaps_accounted_bytes() reads the tally.  Host-side bookkeeping only: nothing is launched, nothing synchronises. */
int uaps_account(int enable);
double uaps_accounted_bytes(void);
/* Zero n floats of bound storage (a multiple of UAPS_BOUND_FLOATS) with agent-scope stores -- the way bounds handed to
 * uaps_call_hints::out_amax must be cleared (a plain fill may be written back over the atomically raised value). */
int uaps_zero_bounds(float* bounds, long n, uaps_stream_t stream);
int uaps_conv_get_mode(void);
/* both packed buffers hold the fp32 layout followed by the bf16-split and the fp16-split layouts; they must be 16-byte aligned */
int uaps_conv_pack_floats(int Cout, int Cin, int ks, size_t* fwd_floats_host, size_t* bwd_floats_host);
int uaps_conv_pack_weights(const float* w, int Cout, int Cin, int ks, float* wf, float* wb, uaps_stream_t stream);
/* n convolutions packed by one launch (host arrays with n entries; wf[i] or wb[i] may be NULL). */
int uaps_conv_pack_weights_batch(const float* const* w_host, float* const* wf_host, float* const* wb_host,
                                 const int* Cout_host, const int* Cin_host, const int* ks_host, int n,
                                 uaps_stream_t stream);
/* y [B,Cout,H,W] = conv2d(x [B,Cin,H,W], w) (+ bias[Cout] if bias != NULL) */
int uaps_conv_fwd(const float* x, const float* wf, const float* bias, float* y, int B, int Cin, int Cout, int H,
                  int W, int ks, int cfg, uaps_stream_t stream);
/* uaps_conv_fwd that also writes the first pass of the BatchNorm that follows (UAPS_unet.py:37-38, 41-42):
 * stats = float2 [Cout][B][parts_per_image] per-tile (sum, sum of squares) of y, parts_per_image from
 * uaps_conv_fwd_stats_parts; consumed by uaps_bn_act_fwd_train_partials. */
int uaps_conv_fwd_stats(const float* x, const float* wf, const float* bias, float* y, void* stats, int B, int Cin,
                        int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream);
int uaps_conv_fwd_stats_parts(int B, int Cin, int Cout, int H, int W, int ks, int cfg, int* parts_per_image_host);
/* dx [B,Cin,H,W] = conv_transpose2d(dy [B,Cout,H,W], w) */
int uaps_conv_bwd_data(const float* dy, const float* wb, float* dx, int B, int Cin, int Cout, int H, int W,
                       int ks, int cfg, uaps_stream_t stream);
/* dw [Cout][Cin][ks][ks] = sum over batch and pixels of dy (x) x ; dbias [Cout] = sum dy (may be NULL).
 * Partial sums per pixel split go to the workspace and are reduced in a fixed order (deterministic). */
int uaps_conv_wrw_workspace_bytes(int B, int Cin, int Cout, int H, int W, int ks, int cfg, size_t* out_host);
/* The two launches of uaps_conv_bwd_weight as separate calls (same workspace, same dims and cfg):
 * the MFMA kernel that writes the per-split partials, then the fixed-order reduction. */
int uaps_conv_bwd_weight_partial(const float* dy, const float* x, int want_bias, int B, int Cin, int Cout, int H, int W,
                                 int ks, int cfg, void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_conv_bwd_weight_reduce(const void* workspace, float* dw, float* dbias, int B, int Cin, int Cout, int H, int W,
                                int ks, int cfg, uaps_stream_t stream);
/* The reductions of SEVERAL weight gradients by one launch (per 28 items): items[i] names what uaps_conv_bwd_weight_reduce would
 * have been called with for gradient i (the workspace its *_partial call wrote, dims and cfg of that call); results are
 * bit-identical to the single calls.  The workspaces must be distinct buffers, untouched between the partial call and this one.
 * A training step has ~60 convolutions; their reductions are 5-6 us launches of latency each (uaps_amd/conv.py: deferred_reduces). */
typedef struct uaps_wrw_reduce_item {
    const void* workspace; float* dw; float* dbias;      /* dbias NULL: the partial call ran with want_bias = 0 */
    int B, Cin, Cout, H, W, ks, cfg;
} uaps_wrw_reduce_item;
int uaps_conv_bwd_weight_reduce_batch(const uaps_wrw_reduce_item* items, int n, uaps_stream_t stream);
/* Convolutions over a channel concatenation that is never materialised: the first ConvBlock conv of an UpBlock
 * reads torch.cat([skip, upsampled], dim=1) (UAPS_unet.py:84-85).  x1 [B,C1,H,W], x2 [B,C2,H,W], weights packed for
 * Cin = C1 + C2 as usual; C1 must be a multiple of 16.  The input gradient comes back as two tensors, and the
 * weight gradient reads the two inputs; uaps_conv_bwd_weight_reduce(.., Cin = C1 + C2, ..) finishes it. */
/* cfg bit UAPS_CONV_X2_UP2 on uaps_conv_fwd_cat / uaps_conv_bwd_weight_partial_cat (round 5): x2 is the LOW-resolution tensor
 * [B, C2, H/2, W/2] of an UpBlock and is bilinearly up-sampled x2 (align_corners = True, ATen's arithmetic: bit-identical to
 * uaps_up_cat_fwd's output) while the kernel stages it -- `self.up(x1)` of UAPS_unet.py:74-75, 83 is never materialised.  bound[1]
 * (forward) / bound[2] (weight gradient) is the bound of the low tensor (interpolation is convex).  Built for the full-width-row
 * kernels of up4's first convolution (16 + 16 -> 16 channels, W == 256, H % 16 == 0, fp16-split arithmetic with every operand
 * bounded); anything else returns UAPS_ENOFORM with nothing launched: call uaps_up_cat_fwd and the plain entry point.  The input
 * gradient (uaps_conv_bwd_data_cat) still yields the gradient of the up-sampled tensor; uaps_up_cat_bwd folds it to [B,C2,H/2,W/2]. */
#define UAPS_CONV_X2_UP2 (1 << 10)
/* cfg bit UAPS_CONV_BOUNDED on uaps_conv_fwd_stats_parts and the forward entry points (round 6): the caller PROMISES that the call's
 * hints carry a magnitude bound for every tensor operand (mode 2).  It lets the planner pick kernels that exist in the fp16-split
 * arithmetic only and write their BatchNorm partial sums in a layout of their own (csrc/conv_split_g.hpp: one part per 4-row band on
 * 32-wide maps): uaps_conv_fwd_stats_parts reports that layout for the same dimensions + bit, and a call that sets the bit without
 * the bounds is UAPS_EINVAL, and so is uaps_conv_fwd_bn with the bit on such a shape (the staging-time BatchNorm form keeps the tile
 * kernels and their layout).  Without the bit nothing changes (calls without statistics choose the kernel from the hints alone). */
#define UAPS_CONV_BOUNDED (1 << 11)
int uaps_conv_fwd_cat(const float* x1, int C1, const float* x2, int C2, const float* wf, const float* bias, float* y,
                      void* stats_or_null, int B, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream);
int uaps_conv_bwd_data_cat(const float* dy, const float* wb, float* dx1, int C1, float* dx2, int C2, int B, int Cout,
                           int H, int W, int ks, int cfg, uaps_stream_t stream);
int uaps_conv_bwd_weight_partial_cat(const float* dy, const float* x1, int C1, const float* x2, int C2, int want_bias,
                                     int B, int Cout, int H, int W, int ks, int cfg, void* workspace,
                                     size_t workspace_bytes, uaps_stream_t stream);
/* conv -> BatchNorm(train) -> LeakyReLU -> conv without the activated tensor in between (the two convs of a ConvBlock,
 * UAPS_unet.py:37-41; an UpBlock's conv1x1 / Decoder.out_conv after a ConvBlock, :73, :138).  uaps_bn_finalize_train turns
 * the first conv's epilogue partials into batch statistics (running statistics updated as nn.BatchNorm2d does) and
 * xf [groups][C] float2 = (scale, shift) = (gamma*invstd, beta - mean*scale); the second conv reads the RAW output y of the
 * first and applies leaky_relu(fma(y, scale, shift)) (0 <= slope <= 1) while staging, in the forward (uaps_conv_fwd_bn) and in its weight gradient
 * (uaps_conv_bwd_weight_partial_bn, finished by uaps_conv_bwd_weight_reduce).  Its input gradient is uaps_conv_bwd_data,
 * followed by uaps_bn_act_bwd_grouped(drop_p = 0) on (that gradient, y).  W % 4 == 0, 16-byte aligned tensors, no
 * dilation, Cin > 4; otherwise UAPS_ERANGE (use the unfused calls). */
int uaps_bn_finalize_train(const void* partials, int parts_per_image, const float* conv_bias, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                           float momentum, float eps, int B, int C, int H, int W, int groups, float* save_mean,
                           float* save_invstd, void* xf, uaps_stream_t stream);
int uaps_conv_fwd_bn(const float* x_raw, const void* xf, float slope, int groups, const float* wf, const float* bias,
                     float* y, void* stats_or_null, int B, int Cin, int Cout, int H, int W, int ks, int cfg,
                     uaps_stream_t stream);
int uaps_conv_bwd_weight_partial_bn(const float* dy, const float* x_raw, const void* xf, float slope, int groups,
                                    int want_bias, int B, int Cin, int Cout, int H, int W, int ks, int cfg,
                                    void* workspace, size_t workspace_bytes, uaps_stream_t stream);
/* ---- Explicit form of the convolution calls (round 5): ONE size-versioned argument struct per call, no side channel -------------
 * The entry points above take their optional operands (magnitude bounds, statistics shift, the pending BatchNorm transform of
 * dy) from uaps_next_call_hints, a one-shot thread-local record: a binding has to know which call consumes it.  uaps_conv_ex
 * carries everything in the struct; nothing set before the call is looked at (pending hints of the thread are dropped) and
 * nothing survives it, so it is re-entrant per call and a foreign-language binding sees every operand in one place.  Same
 * kernels, same results, same return codes (UAPS_ENOFORM for a dyt_* request the layer's kernel cannot honour).
 *   op = UAPS_CONV_FWD            y (and y's BatchNorm partials into `stats` when non-NULL) = conv(x [, x2]); with `xf` non-NULL the
 *                                 input is a raw conv output and leaky_relu(fma(x, scale, shift)) is applied while staging
 *        UAPS_CONV_BWD_DATA       dx (= y [, y2 for a two-tensor input]) = conv_transpose(dy = x)
 *        UAPS_CONV_BWD_WEIGHT     per-split partials into `workspace` from (dy = y_grad, x [, x2]); finish with uaps_conv_bwd_weight_reduce
 *   Fields that an op does not use must be zero.  struct_size = sizeof(uaps_conv_call) of the caller's header; fields are only
 *   appended, a shorter struct of an older client reads as zero beyond its size. */
#define UAPS_CONV_FWD 0
#define UAPS_CONV_BWD_DATA 1
#define UAPS_CONV_BWD_WEIGHT 2
typedef struct uaps_conv_call {
    unsigned struct_size;
    int op;
    int B, Cin, Cout, H, W, ks, cfg;     /* Cin = C1 + C2 for a two-tensor input */
    const float* x;  int C1;             /* first input tensor [B,C1,H,W] (C1 = Cin without x2); BWD_DATA: dy [B,Cout,H,W] */
    const float* x2;                     /* second input tensor [B,Cin-C1,H,W] or NULL */
    const float* w_packed;               /* uaps_conv_pack_weights: wf (FWD), wb (BWD_DATA); unused by BWD_WEIGHT */
    const float* bias;                   /* FWD: [Cout] or NULL */
    float* y;                            /* FWD: output; BWD_DATA: dx (first tensor) */
    float* y2;                           /* BWD_DATA of a two-tensor input: dx of the second tensor */
    const float* y_grad;                 /* BWD_WEIGHT: dy [B,Cout,H,W] */
    void* stats;                         /* FWD: float2 [Cout][B][parts] or NULL (uaps_conv_fwd_stats_parts) */
    const void* xf; float xf_slope; int xf_groups;      /* staging-time BatchNorm + LeakyReLU of x (uaps_bn_finalize_train) or NULL */
    int want_bias;                       /* BWD_WEIGHT: also the bias gradient's partials */
    void* workspace; size_t workspace_bytes;            /* BWD_WEIGHT (uaps_conv_wrw_workspace_bytes) */
    uaps_stream_t stream;                /* ABI 3: in FRONT of the hints -- the record below is the part of this struct that grows, and a
                                          * client built against a shorter uaps_call_hints must still have its stream where the library
                                          * reads it (ABI 2 had it behind the hints) */
    uaps_call_hints hints;               /* the operands' bounds, statistics shift, dyt_* ...; hints.struct_size may be 0 = none, and
                                          * must not exceed what struct_size leaves for it */
} uaps_conv_call;
int uaps_conv_ex(const uaps_conv_call* call);
/* The name (as rocprofv3 prints it, without namespace) of the kernel instantiation uaps_conv_ex(call) launches, nothing launched and
 * no HIP call made: the same struct, resolved exactly as the launch resolves it (data pointers are looked at for their alignment
 * only; the workspace size is not checked).  buf_host needs >= 64 bytes.  A call that has no kernel returns the code uaps_conv_ex
 * would return (UAPS_ENOFORM for a hint no form honours, ...).  bench.py names each timed launch by it. */
int uaps_conv_ex_variant(const uaps_conv_call* call, char* buf_host, size_t buflen);

/* Name (as rocprofv3 prints it, without namespace) of the kernel instantiation the calls above launch
 * for these dimensions with 16-byte aligned tensors and no hints (uaps_conv_ex_variant with null pointers); buf_host needs
 * >= 64 bytes.  For uaps_conv_bwd_data pass Cin and Cout swapped to uaps_conv_fwd_variant. */
int uaps_conv_fwd_variant(int B, int Cin, int Cout, int H, int W, int ks, int cfg, char* buf_host, size_t buflen);
int uaps_conv_wrw_variant(int B, int Cin, int Cout, int H, int W, int ks, int cfg, char* buf_host, size_t buflen);
int uaps_conv_bwd_weight(const float* dy, const float* x, float* dw, float* dbias, int B, int Cin, int Cout, int H,
                         int W, int ks, int cfg, void* workspace, size_t workspace_bytes, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sibling consistency terms on two [B,C,H,W] tensors (C in [2,8]): the formulations the reference keeps beside
 * the UAPS block (utilities/losses_1.py, losses_2.py; star-imported at UAPS_train.py:21-22) and its evaluation
 * notebook uses (UAPS-Testing.ipynb cell 24).  a = input logits (receives the gradient), b = target logits.
 *   mse_map [B,C,H,W] = (softmax(a) - softmax(b))^2                      losses_1.py:9-26  softmax_mse_loss
 *   kl_map  [B,H,W]   = sum_c KLDivLoss('none')(log_softmax(a), softmax(b))   notebook cell 24 uncertainty map
 *   kl_mean [1]       = F.kl_div(log_softmax(a), softmax(b), reduction='mean')  losses_1.py:29-48 softmax_kl_loss
 * Any of the three outputs may be NULL.  With probs != 0 the inputs are probabilities, not logits, and kl_mean is
 * F.kl_div(log(a), b, reduction='mean') = kl_loss(pr=a, gt=b) of losses_2.py:201-213.
 * workspace: uaps_pair_workspace_bytes() (needed for kl_mean only).
 * ------------------------------------------------------------------------------------------- */
int uaps_pair_workspace_bytes(size_t* out_host);
int uaps_softmax_pair_fwd(const float* a, const float* b, int probs, int B, int C, int H, int W, float* mse_map,
                          float* kl_map, float* kl_mean, void* workspace, size_t workspace_bytes, uaps_stream_t stream);
/* d(sum(grad_map * mse_map)) / da   and   d(g * kl_mean) / da  (g = *gscalar, 1 if NULL); b gets no gradient. */
int uaps_softmax_mse_bwd(const float* a, const float* b, const float* grad_map, int B, int C, int H, int W, float* da,
                         uaps_stream_t stream);
int uaps_softmax_kl_bwd(const float* a, const float* b, const float* gscalar, int B, int C, int H, int W, float* da,
                        uaps_stream_t stream);
/* d(sum(grad_map * kl_map)) / da and / db (either may be NULL): the per-pixel KL map differentiated w.r.t. both heads,
 * as UCC weights its pseudo-supervision (UCC/UCC_train.py:213-217, 231-232; neither softmax is detached there). */
int uaps_softmax_klmap_bwd(const float* a, const float* b, const float* grad_map, int B, int C, int H, int W, float* da,
                           float* db, uaps_stream_t stream);
/* entropy_map(p) = -sum_c p log(p + 1e-6) as [B,1,H,W] and/or its mean (entropy_minmization), losses_1.py:139-149. */
int uaps_entropy_map(const float* p, int B, int C, int H, int W, float* ent_map, float* ent_mean, void* workspace,
                     size_t workspace_bytes, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mean Teacher (MT/MT_train.py) and uncertainty-aware Mean Teacher (UAMT/UA_MT_train.py): csrc/loss_mean_teacher.hip.
 * Every tensor below 2 GiB (UAPS_ERANGE otherwise); T in [0, UAPS_MC_MAX_T].
 *
 * uaps_ema_update: update_ema_variables (MT_train.py:79-83) over n (ema, param) pairs of any sizes, one launch per 128 pairs:
 *   ema = ema * alpha + one_minus_alpha * param, the product rounded first (mul_ then add_), alpha = min(1 - 1/(step+1), decay)
 *   and 1 - alpha formed by the caller in double.  Parameters only; BatchNorm buffers are not averaged (as in the reference).
 *
 * uaps_teacher_noise: the (1 + T) B teacher inputs of a UAMT step in one launch, out [(1+T)B, Cin, H, W]:
 *   out[r] = x[r % B] + clamp(0.1f * n, -0.2f, 0.2f)      (UA_MT_train.py:180-181 rows [0,B); :190-194 rows [B,(1+T)B))
 *   n ~ N(0,1): Box-Muller on Philox4x32-10 keyed by `seed`, counter offset + i / 4 for flat element i.  T = 0: the B rows of
 *   MT's teacher input (MT_train.py:181).  _apply: n [(1+T)B, Cin, H, W] given by the caller instead.
 *
 * uaps_mc_consistency_fwd: per pixel of the student logits s and teacher logits e [B,C,H,W]
 *   mc != NULL (mask mode, UA_MT_train.py:194-214): p_bar = mean_t softmax(mc[t]) of the raw MC teacher logits mc [T,B,C,H,W]
 *     (T > 0), or p_bar = mc [B,C,H,W] (T = 0: already-averaged probabilities); u = -sum_c p_bar log(p_bar + 1e-6);
 *     m = u < threshold -> mask uint8 [B,H,W] (required), uncertainty [B,1,H,W] (optional);
 *     out3 = (sum m d / (2 sum m + 1e-16), sum m d, sum m) with d = sum_c (softmax(s) - softmax(e))^2;
 *   mc == NULL (MT mode, MT_train.py:199): out3 = (mean((softmax(s) - softmax(e))^2), sum d, B H W); T must be 0.
 *   workspace: uaps_mc_consistency_workspace_bytes().
 * uaps_mc_consistency_bwd: d(grad[0] * out3[0]) / ds; the teacher gets no gradient.  mask and out3 of the mask-mode forward
 *   (device pointers: no host sync), or both NULL for MT mode.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_MC_MAX_T 16
int uaps_ema_update(float* const* ema_host, const float* const* param_host, const long* numel_host, int n, float alpha,
                    float one_minus_alpha, uaps_stream_t stream);
int uaps_teacher_noise(const float* x, int B, int Cin, int H, int W, int T, uint64_t seed, uint64_t offset, float* out,
                       uaps_stream_t stream);
int uaps_teacher_noise_apply(const float* x, const float* noise, int B, int Cin, int H, int W, int T, float* out,
                             uaps_stream_t stream);
int uaps_mc_consistency_workspace_bytes(size_t* out_host);
int uaps_mc_consistency_fwd(const float* student, const float* teacher, const float* mc, int T, int B, int C, int H, int W,
                            float threshold, uint8_t* mask, float* uncertainty, float* out3, void* workspace, size_t workspace_bytes,
                            uaps_stream_t stream);
int uaps_mc_consistency_bwd(const float* student, const float* teacher, const uint8_t* mask, const float* grad, const float* out3,
                            int B, int C, int H, int W, float* dstudent, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * CCT (CCT/CCT_train.py) and DCT (DCT/DCT_train.py): csrc/loss_cct_dct.hip.  Every tensor below 2 GiB (UAPS_ERANGE otherwise),
 * C in [2, UAPS_MAX_CLASSES] (UAPS_ERANGE), logits fp32 [*, C, H, W] contiguous.  A window [b0, b0 + B) names rows of a larger batch:
 * the kernels read (and the backwards write) those rows only.
 *
 * uaps_cct_consistency_fwd: D in [2, UAPS_CCT_MAX_HEADS] head logits (host array of device pointers; head 0 the main decoder):
 *   out[0] = (1/(D-1)) sum_{k>=1} mean((softmax(z0) - softmax(zk))^2), the mean over the window's B C H W elements
 *   (CCT_train.py:195-200); out[k] = the k-th term's sum (k = 1..D-1).  out: D floats.  Probabilities are never written.
 *   workspace: uaps_cct_dct_workspace_bytes().
 * uaps_cct_consistency_bwd: d(grad[0] * out[0]) / dz for every head (nothing is detached in the reference): with
 *   a = 2 grad[0] / ((D-1) B C H W), g0 = a sum_k (p0 - pk), gk = -a (p0 - pk), dz = p (g - <p, g>), into rows [b0, b0 + B) of the
 *   caller's D gradient buffers (host array of device pointers).  grad is read on the device (no host sync).
 *
 * uaps_rot90_batch: the DCT step's input in one launch (DCT_train.py:165-175): out = [x_l ; x_u ; rot90(x_u, k, [2, 3])] along the
 *   batch axis, x_l and x_u [B, Cin, H, W], k in [0, 3] (UAPS_EINVAL otherwise).  rot_out == NULL: the rotated batch is rows
 *   [2B, 3B) of out (needs k even or H == W); else out holds [x_l ; x_u] and rot_out [B, Cin, Ho, Wo] (Ho, Wo = W, H for odd k).
 *   With uaps_call_hints::out_amax the bound is raised to max|.| of everything written.
 *
 * uaps_rot_consistency_fwd: mean((softmax(r) - rot90(softmax(u), k, [2, 3]))^2) over B C H W (DCT_train.py:188): u = rows
 *   [u_b0, u_b0 + B) of the plain forward's logits [*, C, H, W], r = rows [r_b0, r_b0 + B) of the rotated forward's [*, C, Ho, Wo].
 *   The rotation is an index map inside the kernel.  out2 = (loss, sum).  workspace: uaps_cct_dct_workspace_bytes().
 * uaps_rot_consistency_bwd: d(grad[0] * loss) / dr and / du (both sides trained), written into the same windows of dr and du.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_CCT_MAX_HEADS 8
int uaps_cct_dct_workspace_bytes(size_t* out_host);
int uaps_cct_consistency_fwd(const float* const* heads_host, int D, int b0, int B, int C, int H, int W, float* out, void* workspace,
                             size_t workspace_bytes, uaps_stream_t stream);
int uaps_cct_consistency_bwd(const float* const* heads_host, int D, int b0, int B, int C, int H, int W, const float* grad,
                             float* const* dheads_host, uaps_stream_t stream);
int uaps_rot90_batch(const float* x_l, const float* x_u, int B, int Cin, int H, int W, int k, float* out, float* rot_out,
                     uaps_stream_t stream);
int uaps_rot_consistency_fwd(const float* r, int r_b0, const float* u, int u_b0, int B, int C, int H, int W, int k, float* out2,
                             void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_rot_consistency_bwd(const float* r, int r_b0, const float* u, int u_b0, int B, int C, int H, int W, int k, const float* grad,
                             float* dr, float* du, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * CPS, cross pseudo supervision (CPS/CPS_train.py:195-250): csrc/loss_cps.hip.  z1, z2: fp32 logits [N, C, H, W] (contiguous) of two
 * networks on one batch whose rows [0, B_lab) are labelled (labels int64 [B_lab, H, W]) and rows [B_lab, N) unlabelled;
 * 1 <= B_lab < N (UAPS_EINVAL otherwise), C in [2, UAPS_MAX_CLASSES] (UAPS_ERANGE), every tensor below 2 GiB (UAPS_ERANGE).
 * With CE = nn.CrossEntropyLoss() (mean), Dice = utilities/pytorch_losses.dice_loss (sums over batch and space, mean over the
 * classes, eps) and p_m = the arg-max over the classes of network m's logits, the LOWEST index among equal logits
 * (= torch.argmax(softmax(z_m)) except where the fp32 softmax rounds different logits to one probability), the six terms t are
 *   t = 0, 1   network 1, 2 against the ground truth on the labelled rows                   :215-220
 *   t = 2, 3   network 1 against p_2, network 2 against p_1 on the labelled rows            :228-232
 *   t = 4, 5   the same on the unlabelled rows                                              :238-242
 *   sup = 0.5 (ce_0 + dice_0) + 0.5 (ce_1 + dice_1)                                         :222-224
 *   labeled_cps = 0.5 ce_2 + 0.5 dice_2 + 0.5 ce_3 + 0.5 dice_3                             :231-234
 *   cps = 0.5 ce_4 + 0.5 dice_4 + 0.5 ce_5 + 0.5 dice_5                                     :241-245
 * uaps_cps_fwd: one pass over both tensors + one finalize launch (block partial sums in the workspace, added in double in a fixed
 *   order: deterministic).  scalars: UAPS_CPS_S_NSCALARS(C) floats in the layout below.  pseudo1, pseudo2: optional uint8 [N, H, W]
 *   outputs, the arg-max of z1 / z2 at every pixel (NULL: not stored).  A ground-truth label outside [0, C) enters no term and is
 *   counted in scalars[UAPS_CPS_S_BAD].  workspace: uaps_cps_workspace_bytes().
 * uaps_cps_bwd: one launch overwrites every row of dz1 and dz2: rows [0, B_lab) with d(g_sup sup + g_lcps labeled_cps) / dz, rows
 *   [B_lab, N) with d(g_cps cps) / dz.  g_*: device pointers to one float each, NULL = 1 (read on the device: no host sync).
 *   scalars: what the forward wrote for the same tensors; the pseudo-labels are formed again from the logits (they carry no gradient).
 * ------------------------------------------------------------------------------------------- */
#define UAPS_CPS_S_CE 0                                     /* ce[6]                                              */
#define UAPS_CPS_S_DICE 6                                   /* dice[6]                                            */
#define UAPS_CPS_S_SUP 12
#define UAPS_CPS_S_LCPS 13
#define UAPS_CPS_S_CPS 14
#define UAPS_CPS_S_BAD 15                                   /* number of labels outside [0,C) (must be 0)         */
#define UAPS_CPS_S_A1(C) 16                                 /* [6][C]  2 / (C (card + eps))                       */
#define UAPS_CPS_S_A2(C) (16 + 6 * (C))                     /* [6][C]  2 I / (C (card + eps)^2)                   */
#define UAPS_CPS_S_I(C) (16 + 12 * (C))                     /* [6][C]  Dice intersections  sum p [target = c]     */
#define UAPS_CPS_S_CARD(C) (16 + 18 * (C))                  /* [6][C]  Dice cardinalities  sum p + #[target = c]  */
#define UAPS_CPS_S_NSCALARS(C) (16 + 24 * (C))
int uaps_cps_workspace_bytes(int N, int B_lab, int C, int H, int W, size_t* out_host);
int uaps_cps_fwd(const float* z1, const float* z2, const int64_t* labels, int N, int B_lab, int C, int H, int W, float eps,
                 uint8_t* pseudo1, uint8_t* pseudo2, float* scalars, void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_cps_bwd(const float* z1, const float* z2, const int64_t* labels, const float* scalars, const float* g_sup, const float* g_lcps,
                 const float* g_cps, int N, int B_lab, int C, int H, int W, float* dz1, float* dz2, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * UCC, uncertainty-guided cross-head co-training with cross-cut-mix (UCC/UCC_train.py:147-256, UCC/cross_cutmix.py): csrc/loss_ucc.hip.
 * C in [2, UAPS_MAX_CLASSES] (UAPS_ERANGE), every tensor below 2 GiB (UAPS_ERANGE).
 *
 * uaps_ucc_cutmix_batch: the step's input in one launch.  x_l, x_wk, x_st: fp32 [B, Cin, H, W] (labelled, weakly and strongly augmented
 *   unlabelled batch), y_l int64 [B, H, W]; rects_l, rects_u: HOST arrays of B x 5 int32 (flag, y0, y1, x0, x1), the rectangle
 *   [y0, y1) x [x0, x1) of generate_mix_data / generate_crossmix_data's cut-out mask and whether the image is mixed; 0 <= y0 <= y1 <= H
 *   and 0 <= x0 <= x1 <= W (UAPS_EINVAL otherwise), B <= UAPS_UCC_MAX_BATCH (UAPS_ERANGE): the rectangles travel as kernel arguments,
 *   nothing is copied to the device and nothing waits for it.  With in_1 / in_2 = pixel inside image i's rectangle of list 1 / 2 with
 *   its flag set:   out[i] = in_1 ? x_l[(i+1) % B] : x_l[i] (y_out[i] likewise)          cross_cutmix.py:90-91
 *                   out[B+i] = in_2 ? out[i] : x_wk[i],  out[2B+i] = in_2 ? out[i] : x_st[i]        :115-116 (UCC_train.py:153)
 *   out: [3B, Cin, H, W], y_out: int64 [B, H, W].  Values are selected, so the result equals the reference's a mask + b (1 - mask) as
 *   numbers (a -0.0 stays -0.0 here).  With uaps_call_hints::out_amax the bound is raised to max|out|.
 *
 * z1, z2: fp32 logits [3B, C, H, W] (contiguous) of the two heads, rows [0, B) the mixed labelled batch (labels int64 [B, H, W]),
 * [B, 2B) the weak and [2B, 3B) the strong unlabelled batch.  CE / Dice as for CPS; pseudo_1 = arg-max of z2_wk, pseudo_2 = arg-max of
 * z1_wk over the LOGITS, the lowest index among equals (:224-225).  v1 = sum_c KL(log_softmax z1_wk || softmax z2_st) (:213),
 * v2 likewise from (z1_st, z2_wk) (:216), M = B H W.  Terms t: 0, 1 = head 1, 2 against the labels; 2 = z1_st against pseudo_1;
 * 3 = z2_st against pseudo_2.
 *   sup = 0.5 (ce_0 + dice_0) + 0.5 (ce_1 + dice_1)                                        :197-202
 *   ps_1 = 0.5 (ce_2 + dice_2) mean exp(-v1) + mean v1,  ps_2 = 0.5 (ce_3 + dice_3) mean exp(-v2) + mean v2,  ps = ps_1 + ps_2   :233-240
 * uaps_ucc_fwd: one pass over both tensors + one finalize launch (block partial sums in the workspace, added in double in a fixed
 *   order: deterministic).  scalars: UAPS_UCC_S_NSCALARS(C) floats in the layout below.  Optional outputs (NULL: not stored): pseudo1,
 *   pseudo2 uint8 [B, H, W]; var1, var2 fp32 [B, H, W] = v1, v2.  A label outside [0, C) enters no term and is counted in
 *   scalars[UAPS_UCC_S_BAD].  workspace: uaps_ucc_workspace_bytes().
 * uaps_ucc_bwd: one launch overwrites every row of dz1 and dz2 with d(g_sup sup + g_ps ps) / dz.  g_*: device pointers to one float
 *   each, NULL = 1.  Neither softmax of a KL pair is detached (the reference detaches the pseudo-labels only).
 * ------------------------------------------------------------------------------------------- */
#define UAPS_UCC_MAX_BATCH 64
#define UAPS_UCC_S_CE 0                                     /* ce[4]                                              */
#define UAPS_UCC_S_DICE 4                                   /* dice[4]                                            */
#define UAPS_UCC_S_SUP 8
#define UAPS_UCC_S_PS 9
#define UAPS_UCC_S_PS1 10
#define UAPS_UCC_S_PS2 11
#define UAPS_UCC_S_V1 12                                    /* mean v1                                            */
#define UAPS_UCC_S_E1 13                                    /* mean exp(-v1)                                      */
#define UAPS_UCC_S_V2 14
#define UAPS_UCC_S_E2 15
#define UAPS_UCC_S_BAD 16                                   /* number of labels outside [0,C) (must be 0); 17..19 reserved */
#define UAPS_UCC_S_A1(C) 20                                 /* [4][C]  2 / (C (card + eps))                       */
#define UAPS_UCC_S_A2(C) (20 + 4 * (C))                     /* [4][C]  2 I / (C (card + eps)^2)                   */
#define UAPS_UCC_S_I(C) (20 + 8 * (C))                      /* [4][C]  Dice intersections                         */
#define UAPS_UCC_S_CARD(C) (20 + 12 * (C))                  /* [4][C]  Dice cardinalities                         */
#define UAPS_UCC_S_NSCALARS(C) (20 + 16 * (C))
int uaps_ucc_cutmix_batch(const float* x_l, const float* x_wk, const float* x_st, const int64_t* y_l, const int32_t* rects_l_host,
                          const int32_t* rects_u_host, int B, int Cin, int H, int W, float* out, int64_t* y_out, uaps_stream_t stream);
int uaps_ucc_workspace_bytes(int B, int C, int H, int W, size_t* out_host);
int uaps_ucc_fwd(const float* z1, const float* z2, const int64_t* labels, int B, int C, int H, int W, float eps, uint8_t* pseudo1,
                 uint8_t* pseudo2, float* var1, float* var2, float* scalars, void* workspace, size_t workspace_bytes,
                 uaps_stream_t stream);
int uaps_ucc_bwd(const float* z1, const float* z2, const int64_t* labels, const float* scalars, const float* g_sup, const float* g_ps,
                 int B, int C, int H, int W, float* dz1, float* dz2, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The supervised loss family (utilities/pytorch_losses.py: ce_loss :31-51, dice_loss :54-89, jaccard_loss :92-128, tversky_loss
 * :131-175; utilities/losses_1.py: FocalLoss :63-97, DiceLoss :100-136): csrc/loss_seg.hip.  z: fp32 logits [B, C, H, W] (contiguous),
 * labels int64 [B, H, W]; C in [2, UAPS_MAX_CLASSES] (UAPS_ERANGE), every tensor below 2 GiB (UAPS_ERANGE).
 * With p = softmax(z) over the classes, y the label, nll = -log p_y, valid = (y != ignore_index) and the sums over the valid pixels
 *   A_c = sum p_c,  I_c = sum p_c [y = c],  N_c = #[y = c],  Z_c = sum p_c^2
 * the terms are
 *   ce      = sum w_y nll / sum w_y                      w = class_weight (torch's weight + ignore_index mean; 0/0 = NaN when every
 *                                                        pixel is ignored, as in torch)
 *   focal   = sum a_y (1 - p_y)^gamma nll / n_valid      a = focal_alpha; focal_mean == 0: the sum.  (1 - p_y)^gamma carries no
 *                                                        gradient (the reference detaches p_t, losses_1.py:85)
 *   dice    = 1 - mean_c 2 I_c / (A_c + N_c + eps)
 *   jaccard = 1 - mean_c I_c / (A_c + N_c - I_c + eps)
 *   tversky = 1 - mean_c I_c / (I_c + alpha (A_c - I_c) + beta (N_c - I_c) + eps)
 *   dice_sq = (1 / C) sum_c v_c (1 - (2 I_c + smooth) / (Z_c + N_c + smooth))        v = dice_sq_weight; losses_1.DiceLoss with
 *                                                        softmax=True has smooth = 1e-5
 *   loss    = sum over the terms selected in `terms` of coef[t] * term_t               (t = the bit's index)
 * A defined extension: a pixel whose label equals ignore_index enters NO term (the reference's region losses raise on such a label,
 * torch.eye(C)[true] indexes out of range; its FocalLoss has no ignore_index).  With no ignored pixel every term equals the
 * reference's.  A label outside [0, C) that is not ignore_index enters no term either and is counted in scalars[UAPS_SEG_S_BAD].
 * uaps_segloss_params is passed by value into the kernels: nothing is copied to the device and nothing waits for it.
 * uaps_segloss_fwd: one pass over z (each logit read once) + one finalize launch (block partial sums in the workspace, added in
 *   double in a fixed order: deterministic).  scalars: UAPS_SEG_S_NSCALARS(C) floats in the layout below; a term that is not selected
 *   is stored as 0 (Z_c is accumulated only when dice_sq is selected).
 * uaps_segloss_bwd: one launch overwrites all of dz with grad[0] * d loss / dz (grad: device pointer to one float, NULL = 1, read on
 *   the device); dz = 0 at ignored and at out-of-range pixels.  prm and scalars: what the forward got and wrote for the same tensors.
 * Errors (nothing is launched): UAPS_EINVAL null pointer, non-positive dimension, terms == 0 or a bit outside UAPS_SEG_ALL,
 *   struct_size below the first version's; UAPS_ERANGE; UAPS_EWORKSPACE.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_SEG_CE 1u
#define UAPS_SEG_FOCAL 2u
#define UAPS_SEG_DICE 4u
#define UAPS_SEG_JACCARD 8u
#define UAPS_SEG_TVERSKY 16u
#define UAPS_SEG_DICE_SQ 32u
#define UAPS_SEG_ALL 63u
#define UAPS_SEG_NTERMS 6
typedef struct uaps_segloss_params {
    uint32_t struct_size;                        /* sizeof(uaps_segloss_params) of the caller's header; fields are only ever appended */
    uint32_t terms;                              /* bit mask UAPS_SEG_CE | _FOCAL | _DICE | _JACCARD | _TVERSKY | _DICE_SQ */
    float coef[UAPS_SEG_NTERMS];                 /* coefficient of term t = bit index                                       */
    float class_weight[UAPS_MAX_CLASSES];        /* CE                                                                      */
    float focal_alpha[UAPS_MAX_CLASSES];
    float focal_gamma;
    int focal_mean;                              /* non-zero: divide by the number of valid pixels (size_average)           */
    float dice_sq_weight[UAPS_MAX_CLASSES];
    float tversky_alpha, tversky_beta, eps, smooth;
    int64_t ignore_index;                        /* a value no label takes (e.g. INT64_MIN) = nothing ignored               */
} uaps_segloss_params;
#define UAPS_SEG_S_TERM 0                                   /* term[6]: ce, focal, dice, jaccard, tversky, dice_sq  */
#define UAPS_SEG_S_LOSS 6
#define UAPS_SEG_S_BAD 7                                    /* labels outside [0,C) and != ignore_index (must be 0) */
#define UAPS_SEG_S_NVALID 8                                 /* pixels that entered the terms                        */
#define UAPS_SEG_S_WSUM 9                                   /* sum w_y (0 unless ce is selected)                    */
#define UAPS_SEG_S_KCE 10                                   /* coef_ce / sum w_y               (0: not selected)    */
#define UAPS_SEG_S_KFOCAL 11                                /* coef_focal / n_valid, or coef_focal for the sum      */
#define UAPS_SEG_S_A(C) 16                                  /* [C]  sum p_c                     12..15 reserved     */
#define UAPS_SEG_S_I(C) (16 + (C))                          /* [C]  sum p_c [y = c]                                 */
#define UAPS_SEG_S_N(C) (16 + 2 * (C))                      /* [C]  #[y = c]                                        */
#define UAPS_SEG_S_Z(C) (16 + 3 * (C))                      /* [C]  sum p_c^2                                       */
#define UAPS_SEG_S_GA(C) (16 + 4 * (C))                     /* [C]  d loss / d A_c     backward: d loss / d p_c =   */
#define UAPS_SEG_S_GI(C) (16 + 5 * (C))                     /* [C]  d loss / d I_c       GA_c + [y = c] GI_c        */
#define UAPS_SEG_S_GZ(C) (16 + 6 * (C))                     /* [C]  d loss / d Z_c       + 2 p_c GZ_c               */
#define UAPS_SEG_S_NSCALARS(C) (16 + 7 * (C))
int uaps_segloss_workspace_bytes(int B, int C, int H, int W, size_t* out_host);
int uaps_segloss_fwd(const float* z, const int64_t* labels, const uaps_segloss_params* prm, int B, int C, int H, int W, float* scalars,
                     void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_segloss_bwd(const float* z, const int64_t* labels, const uaps_segloss_params* prm, const float* scalars, const float* grad,
                     int B, int C, int H, int W, float* dz, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One-channel sigmoid (binary) heads (utilities/losses_2.py: FocalLoss :7-26, JaccardLoss, DiceLoss, BCEJaccardLoss, BCEDiceLoss,
 * iou :108-139, f_score :145-180; utilities/pytorch_losses.py: bce_loss :9-28 and the num_classes == 1 branches of dice_loss :70-79,
 * jaccard_loss :108-117, tversky_loss :153-162; utilities/losses_1.py: the sigmoid branches of softmax_mse_loss / softmax_kl_loss):
 * csrc/loss_binary.hip.  z: fp32 logits [B, 1, H, W] (contiguous, below 2 GiB: UAPS_ERANGE).  target: int64 labels [B, H, W] in {0, 1}
 * (target_float == 0) or a float32 soft target in [0, 1] of the logits' shape (target_float != 0; not range-checked).
 * With p = sigmoid(z), g the target, sp = log1p(exp(-|z|)), over the elements that enter (all of a float target; the labels in {0, 1}):
 *   l0 = max(z, 0) - z g + sp                                      F.binary_cross_entropy_with_logits
 *   l  = (1 - g) z + (1 + (w - 1) g) (sp + max(-z, 0))             the same with pos_weight w (has_pos_weight != 0), else l = l0
 *   n = #elements,  P = sum p,  G = sum g,  I = sum g p
 *   bce      = sum l / n
 *   focal    = alpha sum (1 - e^{-l0})^gamma l0 / n                focal_mean == 0: the sum.  e^{-l0} carries its gradient (losses_2.py:20
 *                                                                  does not detach it)
 *   jaccard  = 1 - (I + eps) / (G + P - I + eps)                   losses_2.JaccardLoss
 *   fscore   = 1 - ((1 + b2) I + eps) / ((1 + b2) I + b2 (G - I) + (P - I) + eps),  b2 = beta^2        losses_2.DiceLoss at beta = 1
 *   dice2, jaccard2, tversky2 = the multi-class formulas of uaps_segloss_* averaged over the two channels [pos, neg] with
 *                              I_neg = n - P - G + I,  A_neg = n - P,  N_neg = n - G      (pytorch_losses.py, num_classes == 1)
 *   loss     = sum over the selected terms of coef[t] * term_t     (t = the bit's index)
 * A label outside {0, 1} enters no term and is counted in scalars[UAPS_BIN_S_BAD]; dz is 0 there.  If no label is in range
 *   (n == 0), bce and focal are 0 (not 0 / 0), the region terms are their formulas at all-zero sums, and dz is 0 everywhere.
 * uaps_binloss_fwd: one pass over z + one finalize launch (block partial sums in the workspace, added in double in a fixed order:
 *   deterministic).  scalars: UAPS_BIN_S_NSCALARS floats; a term that is not selected is stored as 0.
 * uaps_binloss_bwd: one launch overwrites dz with grad[0] * d loss / dz =
 *   grad [k_bce ((1 + (w - 1) g) p - w g) + k_focal d focal / dz + p (1 - p) (gP + g gI)]   (grad: device pointer to one float, NULL = 1).
 * Errors (nothing is launched): UAPS_EINVAL null pointer, non-positive dimension, terms == 0 or a bit outside UAPS_BIN_ALL, struct_size
 *   below the first version's; UAPS_ERANGE at 2 GiB; UAPS_EWORKSPACE.
 * uaps_sigmoid_mse_fwd / _bwd: out[i] = (sigmoid(a) - sigmoid(b))^2 over n floats; da = g_map 2 (sigmoid(a) - sigmoid(b)) p_a (1 - p_a).
 * uaps_sigmoid_kl_fwd / _bwd: out_mean = mean t (log t - log sigmoid(a)), t = sigmoid(b), log sigmoid(x) = -softplus(-x) (F.kl_div,
 *   reduction "mean"); da = -grad t (1 - sigmoid(a)) / n.  The gradient goes to a only.  Workspace: uaps_binloss_workspace_bytes.
 * uaps_bin_confusion: counts[2 t + p] (int64 [2][2], overwritten, exact), p = sigmoid(z) > threshold evaluated as
 *   z > (float) logit(threshold), 0 < threshold < 1 (UAPS_EINVAL otherwise); a label outside {0, 1} is not counted.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_BIN_BCE 1u
#define UAPS_BIN_FOCAL 2u
#define UAPS_BIN_JACCARD 4u
#define UAPS_BIN_FSCORE 8u
#define UAPS_BIN_DICE2 16u
#define UAPS_BIN_JACCARD2 32u
#define UAPS_BIN_TVERSKY2 64u
#define UAPS_BIN_ALL 127u
#define UAPS_BIN_NTERMS 7
typedef struct uaps_binloss_params {
    uint32_t struct_size;                        /* sizeof(uaps_binloss_params) of the caller's header; fields are only ever appended */
    uint32_t terms;                              /* bit mask UAPS_BIN_*                                                      */
    float coef[UAPS_BIN_NTERMS];                 /* coefficient of term t = bit index                                        */
    uint32_t target_float;                       /* 0: int64 labels [B,H,W]; non-zero: float32 soft target                   */
    uint32_t has_pos_weight;                     /* non-zero: bce uses pos_weight                                            */
    float pos_weight;
    float focal_alpha, focal_gamma;
    int focal_mean;                              /* non-zero: divide by n (reduce=True)                                      */
    float beta;                                  /* fscore                                                                   */
    float tversky_alpha, tversky_beta, eps;
} uaps_binloss_params;
#define UAPS_BIN_S_TERM 0                        /* term[7]: bce, focal, jaccard, fscore, dice2, jaccard2, tversky2          */
#define UAPS_BIN_S_LOSS 7
#define UAPS_BIN_S_BAD 8                         /* labels outside {0, 1} (must be 0)                                        */
#define UAPS_BIN_S_N 9                           /* elements that entered the terms                                          */
#define UAPS_BIN_S_P 10                          /* sum p                                                                    */
#define UAPS_BIN_S_G 11                          /* sum g                                                                    */
#define UAPS_BIN_S_I 12                          /* sum g p                                                                  */
#define UAPS_BIN_S_GP 13                         /* d loss / dP of the region terms                                          */
#define UAPS_BIN_S_GI 14                         /* d loss / dI                                                              */
#define UAPS_BIN_S_KBCE 15                       /* coef_bce / n                        (0: not selected)                    */
#define UAPS_BIN_S_KFOCAL 16                     /* coef_focal alpha / n, or coef_focal alpha for the sum                    */
#define UAPS_BIN_S_NSCALARS 24                   /* 17..23 reserved (stored as 0)                                            */
int uaps_binloss_workspace_bytes(int B, int H, int W, size_t* out_host);
int uaps_binloss_fwd(const float* z, const void* target, const uaps_binloss_params* prm, int B, int H, int W, float* scalars,
                     void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_binloss_bwd(const float* z, const void* target, const uaps_binloss_params* prm, const float* scalars, const float* grad,
                     int B, int H, int W, float* dz, uaps_stream_t stream);
int uaps_sigmoid_mse_fwd(const float* a, const float* b, long n, float* out, uaps_stream_t stream);
int uaps_sigmoid_mse_bwd(const float* a, const float* b, const float* g_map, long n, float* da, uaps_stream_t stream);
int uaps_sigmoid_kl_fwd(const float* a, const float* b, long n, float* out_mean, void* workspace, size_t workspace_bytes,
                        uaps_stream_t stream);
int uaps_sigmoid_kl_bwd(const float* a, const float* b, const float* grad, long n, float* da, uaps_stream_t stream);
int uaps_bin_confusion(const float* z, const int64_t* labels, int B, int H, int W, double threshold, int64_t* counts,
                       uaps_stream_t stream);

/* Residual join of the ResNet blocks (utilities/resnet.py:47-50, 88-91): out = relu(a + b) over n floats; the
 * backward of both addends is dx = dout * (out > 0).  A NaN sum stays NaN, as torch.relu keeps it (and as the max-pool kernels
 * propagate it); every other sum that is not above 0, -0.0 included, gives +0.0.  uaps_call_hints::out_amax is raised to the
 * maximum of the outputs that are numbers: a NaN output does not enter it. */
int uaps_add_relu(const float* a, const float* b, float* out, long n, uaps_stream_t stream);
int uaps_relu_bwd(const float* dout, const float* out, float* dx, long n, uaps_stream_t stream);
/* BatchNorm(train) + LeakyReLU backward in two halves (no dropout).  `prepare`: the reductions -- coef [groups][C][8] floats =
 * (mean, invstd, gamma invstd, beta, mean(d), mean(d x_hat), 0, 0), dgamma, dbeta, the zero gradient of a conv bias in front
 * (dconv_bias may be NULL) -- and the zeroed bound dy_bound raised to an upper bound of |dy|.  dy itself is then formed by the
 * weight-gradient kernel of the convolution in front (uaps_call_hints::dyt_*) or by `apply` (uaps_call_hints::out_amax
 * honoured); both give what uaps_bn_act_bwd_grouped writes.  Workspace: uaps_bn_workspace_bytes. */
int uaps_bn_act_bwd_prepare(const float* dout, const float* y, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, float slope, int B, int C, int H, int W, int groups, float* coef,
                            float* dgamma, float* dbeta, float* dconv_bias, float* dy_bound, void* workspace, size_t workspace_bytes,
                            uaps_stream_t stream);
int uaps_bn_act_bwd_finalize(const void* partials, int parts_per_image, const float* maxes, const float* gamma, const float* beta,
                             const float* save_mean, const float* save_invstd, int B, int C, int H, int W, int groups, float* coef,
                             float* dgamma, float* dbeta, float* dconv_bias, float* dy_bound, uaps_stream_t stream);
int uaps_bn_act_bwd_apply(const float* dout, const float* y, const float* coef, float slope, int B, int C, int H, int W, int groups,
                          float* dy, uaps_stream_t stream);
/* The backward of a decoder's class convolution and the reductions of the BatchNorm in front of it as ONE pass (csrc/head_bwd_row.hip)
 * where uaps_conv_bwd_data, uaps_conv_bwd_weight_partial_bn and the sums pass of uaps_bn_act_bwd_prepare ran one after the other.
 * dlogits [B,Cout,H,W] is the gradient of z = conv(leaky_relu(batch_norm_train(y)), w) with y [B,Cin,H,W] the raw output of the
 * convolution in front and xf [groups][Cin] float2 (scale, shift) from uaps_bn_finalize_train; wb the packed input-gradient weights
 * of w (uaps_conv_pack_weights).  Written: g [B,Cin,H,W] = d(activation), bit-identical to uaps_conv_bwd_data's; the per-split
 * slabs of dw (and dbias with want_bias) in the workspace layout uaps_conv_wrw_workspace_bytes(B, Cin, Cout, H, W, ks, cfg) reports,
 * for uaps_conv_bwd_weight_reduce[_batch]; partials float2 [Cin][B][H / 16] = (sum d, sum d x_hat) per 16-row run and maxes = two
 * bounds (2 * UAPS_BOUND_FLOATS floats, zeroed by the caller with uaps_zero_bounds) raised to max|d| and max|x_hat|, for
 * uaps_bn_act_bwd_finalize(partials, H / 16, maxes, ...).  dy_bound / x_bound (times their host factors) bound |dlogits| and the
 * activation, as uaps_call_hints::bound[0 / 1] of the weight gradient.  Only enqueues on `stream`; no float atomics, two launches
 * give the same bits.
 * One form: ks == 3, Cin == 16, Cout <= 4, W == 256, H % 16 == 0, mode 2 (fp16-split arithmetic) with both bounds present, 16-byte
 * aligned tensors, cfg without dilation / exact / split bits.  Anything else returns UAPS_ENOFORM with nothing launched: make the
 * three separate calls. */
int uaps_head_bwd_fused(const float* dlogits, const float* y, const void* xf, float slope, int groups, const float* wb,
                        const float* dy_bound, float dy_mul, const float* x_bound, float x_mul, const float* save_mean,
                        const float* save_invstd, const float* gamma, const float* beta, int want_bias, int B, int Cin, int Cout,
                        int H, int W, int ks, int cfg, float* g, void* partials, float* maxes, void* workspace,
                        size_t workspace_bytes, uaps_stream_t stream);

/* The backward of the second convolution of a decoder ConvBlock and the reductions of the BatchNorm in front of it as ONE pass
 * (csrc/mid_bwd_row.hip) where uaps_conv_bwd_weight_partial_bn with uaps_call_hints::dyt_*, uaps_conv_bwd_data and the sums pass of
 * uaps_bn_act_bwd_prepare ran one after the other.  dact [B,Cout,H,W] is the gradient behind the BatchNorm + LeakyReLU that follows
 * z = conv(leaky_relu(batch_norm_train(y1)), w), its transform pending: y2 = z [B,Cout,H,W] raw, coef [groups2][Cout][8] from
 * uaps_bn_act_bwd_prepare / _finalize, slope2 that LeakyReLU's slope; y1 [B,Cin,H,W] is the raw output of the convolution in front and
 * xf [groups][Cin] float2 (scale, shift) from uaps_bn_finalize_train; wb the packed input-gradient weights of w.  The true dz is formed
 * on the way and NOT written.  Written: g [B,Cin,H,W] = d(activation), bit-identical to uaps_conv_bwd_data's on the written-through
 * dz; the per-split slabs of dw (and dbias with want_bias) in the workspace layout uaps_conv_wrw_workspace_bytes(B, Cin, Cout, H, W,
 * ks, cfg) reports, bit-identical to uaps_conv_bwd_weight_partial_bn's; partials float2 [Cin][B][H / 16] and maxes (two bounds, zeroed
 * by the caller) as uaps_head_bwd_fused writes them, for uaps_bn_act_bwd_finalize(partials, H / 16, maxes, ...).  dy_bound / x_bound
 * (times their host factors) bound |dz| and the activation.  Only enqueues on `stream`; no float atomics, two launches give the same
 * bits.
 * One form: ks == 3, Cin == Cout == 16, W == 256, H % 16 == 0, mode 2 (fp16-split arithmetic) with both bounds present, a pending
 * transform (y2 and coef), 16-byte aligned tensors, cfg without dilation / exact / split bits, the row weight-gradient kernels not
 * tuned off.  Anything else returns UAPS_ENOFORM with nothing launched: make the three separate calls. */
int uaps_mid_bwd_fused(const float* dact, const float* y2, const float* coef, float slope2, int groups2, const float* y1,
                       const void* xf, float slope, int groups, const float* wb, const float* dy_bound, float dy_mul,
                       const float* x_bound, float x_mul, const float* save_mean, const float* save_invstd, const float* gamma,
                       const float* beta, int want_bias, int B, int Cin, int Cout, int H, int W, int ks, int cfg, float* g,
                       void* partials, float* maxes, void* workspace, size_t workspace_bytes, uaps_stream_t stream);

/* The input gradient of up4's first convolution with the fold of its up-sampled half as ONE pass (csrc/up_bwd_row.hip) where
 * uaps_conv_bwd_data_cat and uaps_up_cat_bwd(dx2, NULL, dlow, B, 0, C2, H / 2, W / 2) ran one after the other: dy [B,Cout,H,W] is the
 * gradient of conv(cat([skip, up2x(low)]), w), wb the packed input-gradient weights of w, dy_bound (times dy_mul) bounds |dy| as
 * uaps_call_hints::bound[0] of uaps_conv_bwd_data_cat.  Written: dskip [B,C1,H,W], bit-identical to that call's dx1, and dlow
 * [B,C2,H/2,W/2], equal to the two calls' result for finite gradients up to the sign of a zero (the fold leaves out the candidates of
 * weight 0); the full-resolution gradient of the up-sampled tensor is not written.  A non-finite gradient raises
 * UAPS_ERR_CONV_NONFINITE in the error word.  Only enqueues on `stream`; no float atomics, two launches give the same bits.
 * One form: ks == 3, Cout == C1 == C2 == 16, W == 256, H % 16 == 0, mode 2 (fp16-split arithmetic) with the bound present, 16-byte
 * aligned tensors, cfg 0 (UAPS_CONV_BOUNDED ignored), the full-width-row kernels not tuned off, and a size for which
 * uaps_up_bwd_fused_form answers UAPS_OK.  Anything else returns UAPS_ENOFORM with nothing launched: make the two separate calls. */
int uaps_up_bwd_fused(const float* dy, const float* wb, const float* dy_bound, float dy_mul, float* dskip, int C1, float* dlow, int C2,
                      int B, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream);
/* Host only.  The float32 index rule of the x2 align_corners interpolation from n_in to 2 n_in samples (src = mul_rn(r, o),
 * i0 = (int)src, i1 = i0 + (i0 < n_in - 1), weights 1 - frac and frac): the smallest and largest o - 2 i over every pair (output
 * index o, input index i) of non-zero weight.  (-1, 2) is the four-tap support 2 i - 1 .. 2 i + 2 that uaps_up_bwd_fused needs. */
int uaps_up_fold_support(int n_in, int* min_offset, int* max_offset);
/* Host only.  UAPS_OK where the size (H, W) of dy is inside uaps_up_bwd_fused's form (W == 256, H % 16 == 0, four-tap support along
 * both axes), else UAPS_ENOFORM. */
int uaps_up_bwd_fused_form(int H, int W);
/* Host only.  The number of workgroups uaps_up_bwd_fused launches for B images of H rows (each walks its share of the B * H / 16 runs). */
int uaps_up_bwd_fused_grid(int B, int H);

/* The same when the join's output had k <= 4 consumers: dx = (dout[0] + ... + dout[k-1]) * (out > 0), the k gradients (host
 * array of device pointers) summed in order by this pass instead of by k - 1 accumulation passes in front of it. */
int uaps_relu_bwd_sum(const float* const* dout_host, int k, const float* out, float* dx, long n, uaps_stream_t stream);

/* The two batches of a training step as one tensor (the reference runs model(labelled) and model(unlabelled) one after the other,
 * UAPS_train.py:177 and :185; this build runs them as one pass over both): out [2n] = a [n] followed by b [n].  With
 * uaps_call_hints::out_amax the bound is raised to max|out| on the way. */
int uaps_cat2(const float* a, const float* b, float* out, long n, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Input pipeline: the per-sample work of the reference's training loader (utilities/dataloaders.py:60-119: albumentations
 * Resize(nearest) / flips / RandomBrightnessContrast / Blur / RandomRotate90 / GaussNoise, then ToTensor + Normalize; the
 * mask follows the geometry and becomes int64) on a decoded uint8 batch in device memory.
 *   images_hwc [B][Hs][Ws][3] uint8 (RGB, as cv2.cvtColor leaves it), masks [B][Hs][Ws] uint8 or NULL
 *   params_i   [B][8] int32 : hflip, vflip, rot_k (np.rot90 count), blur_k (0 / 3 / 5 / 7), noise_on, reserved x3
 *   params_f   [B][4] float : alpha (contrast factor), beta (brightness shift / 255), sigma (noise std, grey levels), reserved
 *   noise      [B][3][Ho][Wo] float already scaled by sigma, or NULL: drawn in the kernel (Philox, Box-Muller) from `seed`
 *   out        [B][3][Ho][Wo] float normalised with mean3_host / std3_host; out_mask [B][Ho][Wo] int64 (NULL with masks)
 * rot_k odd needs Ho == Wo.  Parity unpinned (cv2 / albumentations are not in the build image): see csrc/augment.hip.
 * ------------------------------------------------------------------------------------------- */
int uaps_augment_batch(const uint8_t* images_hwc, const uint8_t* masks, const int* params_i, const float* params_f,
                       const float* noise, uint64_t seed, int B, int Hs, int Ws, int Ho, int Wo, const float* mean3_host,
                       const float* std3_host, float* out, int64_t* out_mask, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Input pipeline, any recipe, one or two views per source (csrc/augment_views.hip): the dataset variants of the reference's
 * loaders (DAGM / KoSDD2 / MTiles UAPS_dataloaders.py, UCC/UCC_dataloaders.py:149-168) differ in the ORDER of their stages, in the
 * channel count and in the stages they use, so the gather kernel runs a small program per (view, image).  PARITY UNPINNED, as
 * above: the arithmetic is the one written down here, not a measured equality with cv2 / albumentations.
 *
 * Geometry comes first, as one coordinate map: frame = rot90^rot_k(vflip(hflip(resize_nearest(source)))), the "working frame"
 * [Ho][Wo] (rot_k odd needs Ho == Wo).  The program then runs in that frame, on uint8 grey levels held as float; every op ends
 * in a clip to 0..255.  uaps_view_row::op[i] with its operands a[i], b[i]; UAPS_AUG_END (0) ends the program:
 *   UAPS_AUG_BC        trunc(clip(v * a + b * 255))                                    (uaps_augment_batch's line)
 *   UAPS_AUG_NOISE     trunc(clip(v + g)); g = noise[view][image][channel][y][x] (already scaled by sigma) or, without a field,
 *                      a * N(0,1) from Philox + Box-Muller keyed by (seed, op index, view, image, pixel)
 *   UAPS_AUG_BLUR      a = k in {3, 5, 7}: rint(mean of the k x k window), BORDER_REFLECT_101, half to even
 *   UAPS_AUG_BRIGHT    trunc(clip(v * a))
 *   UAPS_AUG_CONTRAST  trunc(clip(v * a + m * (1 - a))), m = rint(mean over the frame of grey) of the image as it enters the
 *                      op, grey = (299 R + 587 G + 114 B) / 1000 (the channel itself when Cs == 1); computed by a pre-pass in
 *                      integers, fixed-order two-stage reduction, so m is exact and deterministic
 *   UAPS_AUG_SATURATE  rint(clip(grey + a * (v - grey))), grey = 0.299 R + 0.587 G + 0.114 B in float; identity when Cs == 1
 *   UAPS_AUG_HUE       hexcone RGB -> HSV in float, H <- frac(H + a), back, rint, clip; identity when Cs == 1
 *   UAPS_AUG_PIXDROP   u = drop_u[view][image][y][x] or one Philox uniform per pixel; all channels 0 where u < a; mask untouched
 *   UAPS_AUG_GRID      the frame is resampled: pixel (y, x) becomes the bilinear sample (float weights, reflect-101 indices,
 *                      rint) at (grid_ys[view][image][y], grid_xs[view][image][x]), positions clamped to the frame; the mask
 *                      takes the node nearest to that position (rint).  uaps_view_row::grid_on must be set exactly when the
 *                      program holds this op.
 * GRID and BLUR split a program into three segments: ops before GRID are evaluated at the four bilinear corners, ops between
 * GRID and BLUR at every blur tap, ops after BLUR once.  Forms that do not exist (UAPS_ENOFORM, nothing launched): NOISE or
 * PIXDROP ahead of GRID, BLUR ahead of GRID, more than one GRID / BLUR, and more than one CONTRAST (the second one's mean would
 * need the first one's pre-pass to have finished inside its own).
 *
 * Every operand travels in one size-versioned struct (fields are only ever appended; struct_size = sizeof of the caller's header).
 * rows_host and rows are the SAME [V][B] rows on the host (read here, for validation and planning only) and on the device (read
 * by the kernels).  workspace: uaps_augment_views_workspace_bytes, needed only when a program holds CONTRAST (NULL / 0 otherwise);
 * on return of the stream's work its first V * B floats hold m per (view, image), -1 where the program has no CONTRAST.
 * The call does not synchronise.  Errors (nothing launched): UAPS_EINVAL null pointer, dimension, V outside {1, 2}, Cs outside
 * {1, 3}, unknown op, blur size, rot_k, grid_on without maps; UAPS_ERANGE V * B > 65535 or a frame beyond 2^31 - 1 pixels; UAPS_EWORKSPACE.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_AUG_END 0
#define UAPS_AUG_BC 1
#define UAPS_AUG_NOISE 2
#define UAPS_AUG_BLUR 3
#define UAPS_AUG_BRIGHT 4
#define UAPS_AUG_CONTRAST 5
#define UAPS_AUG_SATURATE 6
#define UAPS_AUG_HUE 7
#define UAPS_AUG_PIXDROP 8
#define UAPS_AUG_GRID 9
#define UAPS_AUG_MAX_OPS 8
typedef struct uaps_view_row {
    int32_t hflip, vflip, rot_k, grid_on;        /* the geometry row */
    int32_t op[UAPS_AUG_MAX_OPS];                /* the program, executed in order */
    float a[UAPS_AUG_MAX_OPS], b[UAPS_AUG_MAX_OPS];
} uaps_view_row;
typedef struct uaps_augment_views_call {
    uint32_t struct_size;
    int32_t V, B, Hs, Ws, Cs, Ho, Wo;
    const uint8_t* images;                       /* [B][Hs][Ws][Cs] */
    const uint8_t* masks;                        /* [B][Hs][Ws] or NULL */
    const uaps_view_row* rows_host;              /* [V][B], host */
    const uaps_view_row* rows;                   /* [V][B], device, same contents */
    const float* grid_ys;                        /* [V][B][Ho] device, or NULL when no row has grid_on */
    const float* grid_xs;                        /* [V][B][Wo] */
    const float* noise;                          /* [V][B][Cs][Ho][Wo] device or NULL */
    const float* drop_u;                         /* [V][B][Ho][Wo] device or NULL */
    uint64_t seed;
    float mean[3], std[3];                       /* the first Cs are used */
    float* out;                                  /* [V][B][Cs][Ho][Wo] */
    int64_t* out_mask;                           /* [V][B][Ho][Wo], NULL exactly when masks is */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_augment_views_call;
int uaps_augment_views_workspace_bytes(int V, int B, int Ho, int Wo, size_t* bytes);
int uaps_augment_views(const uaps_augment_views_call* call);

/* ---------------------------------------------------------------------------------------------
 * Optimizer: torch.optim.Adam(model.parameters(), lr) of UAPS_train.py:112, stepped at :292 -- one multi-tensor
 * launch per 48 tensors instead of PyTorch's per-chunk foreach kernels.  Host arrays of n device pointers / sizes;
 * `step` is the 1-based step count (bias corrections 1 - beta^step are computed on the host in double).
 * weight_decay is the L2 form of torch.optim.Adam (added to the gradient); amsgrad / maximize are not supported.
 * ------------------------------------------------------------------------------------------- */
int uaps_adam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                   float* const* exp_avg_sq_host, const long* numel_host, int n, double lr, double beta1, double beta2,
                   double eps, double weight_decay, long step, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Metrics: utilities/metrics.py:8-61 (pixel_accuracy, mIoU, mDice) need only the C x C confusion
 * matrix of arg-max(logits) against the labels: counts[t*C + p], int64, overwritten.
 * ------------------------------------------------------------------------------------------- */
int uaps_seg_confusion(const float* logits, const int64_t* labels, int B, int C, int H, int W,
                       int64_t* counts, uaps_stream_t stream);

/* ---- Explicit-hints forms (round 6, ABI 3) -------------------------------------------------------------------------------------
 * `<name>_h(hints, args...)` == `<name>(args...)` with `hints` (NULL or struct_size 0 = none) instead of the thread's pending
 * uaps_next_call_hints record, which is neither read nor cleared.  Same kernels, same results, same return codes; the record is
 * copied size-versioned like uaps_next_call_hints does.  These are what uaps_amd/ (ctypes) binds. */
int uaps_conv_fwd_h(const uaps_call_hints* hints, const float* x, const float* wf, const float* bias, float* y, int B, int Cin, int Cout,
                    int H, int W, int ks, int cfg, uaps_stream_t stream);
int uaps_conv_fwd_stats_h(const uaps_call_hints* hints, const float* x, const float* wf, const float* bias, float* y, void* stats, int B,
                          int Cin, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream);
int uaps_conv_fwd_bn_h(const uaps_call_hints* hints, const float* x_raw, const void* xf, float slope, int groups, const float* wf,
                       const float* bias, float* y, void* stats, int B, int Cin, int Cout, int H, int W, int ks, int cfg,
                       uaps_stream_t stream);
int uaps_conv_fwd_cat_h(const uaps_call_hints* hints, const float* x1, int C1, const float* x2, int C2, const float* wf, const float* bias,
                        float* y, void* stats, int B, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream);
int uaps_conv_bwd_data_h(const uaps_call_hints* hints, const float* dy, const float* wb, float* dx, int B, int Cin, int Cout, int H, int W,
                         int ks, int cfg, uaps_stream_t stream);
int uaps_conv_bwd_data_cat_h(const uaps_call_hints* hints, const float* dy, const float* wb, float* dx1, int C1, float* dx2, int C2, int B,
                             int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream);
int uaps_conv_bwd_weight_partial_h(const uaps_call_hints* hints, const float* dy, const float* x, int want_bias, int B, int Cin, int Cout,
                                   int H, int W, int ks, int cfg, void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_conv_bwd_weight_partial_bn_h(const uaps_call_hints* hints, const float* dy, const float* x_raw, const void* xf, float slope,
                                      int groups, int want_bias, int B, int Cin, int Cout, int H, int W, int ks, int cfg,
                                      void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_conv_bwd_weight_partial_cat_h(const uaps_call_hints* hints, const float* dy, const float* x1, int C1, const float* x2, int C2,
                                       int want_bias, int B, int Cout, int H, int W, int ks, int cfg, void* workspace,
                                       size_t workspace_bytes, uaps_stream_t stream);
int uaps_bn_act_fwd_train_partials_h(const uaps_call_hints* hints, const void* partials, int parts_per_image, const float* y,
                                     const float* conv_bias, const float* gamma, const float* beta, float* running_mean,
                                     float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float slope,
                                     float drop_p, uint64_t seed, uint64_t offset, int B, int C, int H, int W, int groups, float* out,
                                     float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_bn_finalize_train_h(const uaps_call_hints* hints, const void* partials, int parts_per_image, const float* conv_bias,
                             const float* gamma, const float* beta, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, float momentum, float eps, int B, int C, int H, int W, int groups,
                             float* save_mean, float* save_invstd, void* xf, uaps_stream_t stream);
int uaps_bn_act_bwd_grouped_h(const uaps_call_hints* hints, const float* dout, const float* y, const float* gamma, const float* beta,
                              const float* save_mean, const float* save_invstd, float slope, float drop_p, uint64_t seed,
                              uint64_t offset, int B, int C, int H, int W, int groups, float* dy, float* dgamma, float* dbeta,
                              void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_bn_act_bwd_grouped_bias_h(const uaps_call_hints* hints, const float* dout, const float* y, const float* gamma, const float* beta,
                                   const float* save_mean, const float* save_invstd, float slope, float drop_p, uint64_t seed,
                                   uint64_t offset, int B, int C, int H, int W, int groups, float* dy, float* dgamma, float* dbeta,
                                   float* dconv_bias, void* workspace, size_t workspace_bytes, uaps_stream_t stream);
int uaps_bn_act_bwd_apply_h(const uaps_call_hints* hints, const float* dout, const float* y, const float* coef, float slope, int B, int C,
                            int H, int W, int groups, float* dy, uaps_stream_t stream);
/* Encoder glue.  Three forms that spare the encoder's serial phases a launch and a tensor read each; every result is the
 * bits the separate launches produce.  Outside its form each returns UAPS_ENOFORM with nothing launched and nothing written.
 * uaps_bn_act_fwd_train_partials_pool_h: uaps_bn_act_fwd_train_partials_h (no dropout, no residual) whose apply pass also writes
 *   MaxPool2d(2) of the activated tensor -- pooled [B,C,H/2,W/2] and idx uint8 of that shape, exactly what uaps_maxpool2x2_fwd would
 *   make of `out`.  Form: uaps_bn_apply_pool_support(H, W) == UAPS_OK (H even, W % 8 == 0, 4096 % (2 W) == 0), 16-byte aligned
 *   y / out / pooled, 4-byte aligned idx.
 * uaps_fanin_perturbed_bn_sums_h: uaps_fanin_perturbed for a feature map that a train-mode BatchNorm + LeakyReLU (no dropout)
 *   produced from the raw conv output y; the same pass also forms that BatchNorm's backward sums over (out, y): partials float2
 *   [C][B][ceil(H W / 4096)].  Form: what uaps_fanin_perturbed takes, 16-byte aligned y, 8-byte aligned partials, B C <= 65535.
 * uaps_bn_act_bwd_partials_h: the dx pass of uaps_bn_act_bwd_grouped_bias_h alone, from such partials (dconv_bias may be NULL). */
int uaps_bn_apply_pool_support(int H, int W);
int uaps_bn_act_fwd_train_partials_pool_h(const uaps_call_hints* hints, const void* partials, int parts_per_image, const float* y,
                                          const float* conv_bias, const float* gamma, const float* beta, float* running_mean,
                                          float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float slope,
                                          float drop_p, uint64_t seed, uint64_t offset, int B, int C, int H, int W, int groups, float* out,
                                          float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                                          uaps_stream_t stream, float* pooled, uint8_t* idx);
int uaps_fanin_perturbed_bn_sums_h(const uaps_call_hints* hints, const float* const* g_host, const int* mode_host,
                                   const uint8_t* const* keep_host, const uint64_t* offsets_host, int n, int groups, uint64_t seed,
                                   float range, float p, int B, int C, int H, int W, float* out, const float* y, const float* gamma,
                                   const float* beta, const float* save_mean, const float* save_invstd, float slope, void* partials,
                                   uaps_stream_t stream);
int uaps_bn_act_bwd_partials_h(const uaps_call_hints* hints, const void* partials, int parts_per_image, const float* dout, const float* y,
                               const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, float slope, int B,
                               int C, int H, int W, int groups, float* dy, float* dgamma, float* dbeta, float* dconv_bias,
                               uaps_stream_t stream);
int uaps_up_cat_fwd_h(const uaps_call_hints* hints, const float* skip, const float* low, float* out, int B, int Cs, int Cl, int h, int w,
                      uaps_stream_t stream);
int uaps_cat2_h(const uaps_call_hints* hints, const float* a, const float* b, float* out, long n, uaps_stream_t stream);
int uaps_add_relu_h(const uaps_call_hints* hints, const float* a, const float* b, float* out, long n, uaps_stream_t stream);
int uaps_rot90_batch_h(const uaps_call_hints* hints, const float* x_l, const float* x_u, int B, int Cin, int H, int W, int k, float* out,
                       float* rot_out, uaps_stream_t stream);
int uaps_ucc_cutmix_batch_h(const uaps_call_hints* hints, const float* x_l, const float* x_wk, const float* x_st, const int64_t* y_l,
                            const int32_t* rects_l_host, const int32_t* rects_u_host, int B, int Cin, int H, int W, float* out,
                            int64_t* y_out, uaps_stream_t stream);
int uaps_pairloss_bwd_h(const uaps_call_hints* hints, const float* const* lab_logits_host, const float* const* un_logits_host,
                        const int64_t* labels, const int64_t* pseudo, const float* sup_scalars, const float* unsup_scalars, float cw1,
                        float cw2, const float* grad_scale, int D, int B, int C, int H, int W, long n_pixels_loss,
                        float* const* dlab_host, float* const* dun_host, int cfg, uaps_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Test-time augmentation (utilities/base.py:24-46, BaseNet.forward(x, tta=True)): csrc/tta.hip.  Over the scales, and per scale over
 * {plain, horizontally flipped}, the reference resizes the batch (bilinear, align_corners=True), runs the network, takes the softmax,
 * un-flips, resizes back to the input's size and adds: the SUM of S * (1 + flip) probability maps, fp32, accumulated left to right.
 * The bilinear arithmetic is torch's fp32 form: r = (in - 1) / (out - 1) as a float (0 when out == 1), src = r * dst, i0 = (int) src,
 * i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, value = l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11).
 *
 * uaps_tta_views, the input side of one scale: x [B, Cin, H, W] is read once, out [(1 + flip) B, Cin, h, w] receives the resized
 *   batch in images 0 .. B-1 and, with flip == 1, its horizontal flip in images B .. 2B-1 (out[B + b, :, y, j] = out[b, :, y, w-1-j],
 *   the same values stored mirrored), so that ONE forward of 2B images serves both views of the scale.
 * uaps_tta_fold, the output side of all scales in one launch: logits[s] [(1 + flip) B, C, h[s], w[s]] are the network's outputs on the
 *   views of scale s, plain images first.  Per output pixel and per scale, plain then flipped: the softmax over the classes of the
 *   logits at the four source corners, mixed bilinearly, added to C running sums held in registers -- ((((p0 + f0) + p1) + f1) + ...).
 *   The flipped half is un-flipped before its resize: the output column whose neighbours are x0, x1 reads columns w[s] - 1 - x0 and
 *   w[s] - 1 - x1 of image B + b.  Written at the end, whichever are not NULL:
 *     probs_sum [B, C, H, W] the sum;  mask [B, H, W] int64 its arg-max, the lowest index among equal sums;
 *     conf [B, H, W] the largest sum / (S * (1 + flip)).
 *   No atomics and no cross-lane sums: two runs give the same bits.  With W % 4 == 0 and 16-byte aligned outputs a lane owns four
 *   consecutive pixels and stores 16 bytes; otherwise one pixel -- the same arithmetic per pixel either way.
 * Both structs are size-versioned (fields are only ever appended; struct_size = sizeof of the caller's header; a larger one is accepted
 * and what it appends is not read).  The pointer and size tables travel as kernel arguments: no copy, no synchronisation.
 * Errors (nothing launched): UAPS_EINVAL null struct, x / out / logits[s] pointer, all three outputs NULL, non-positive dimension,
 *   struct_size below this version's, flip outside {0, 1}; UAPS_ERANGE C outside [2, UAPS_MAX_CLASSES] (one-channel sigmoid heads
 *   have no form here), S outside [1, UAPS_TTA_MAX_SCALES], a tensor of 2 GiB or more (by dimensions; of the outputs
 *   only those that are not NULL count).
 * ------------------------------------------------------------------------------------------- */
typedef struct uaps_tta_views_call {
    uint32_t struct_size;
    int32_t B, Cin, H, W, h, w, flip;
    const float* x;                              /* [B][Cin][H][W] */
    float* out;                                  /* [(1 + flip) B][Cin][h][w] */
    uaps_stream_t stream;
} uaps_tta_views_call;
int uaps_tta_views(const uaps_tta_views_call* call);

#define UAPS_TTA_MAX_SCALES 8
typedef struct uaps_tta_fold_call {
    uint32_t struct_size;
    int32_t S, B, C, H, W, flip;
    const float* logits[UAPS_TTA_MAX_SCALES];    /* device, [(flip ? 2 : 1) * B, C, h[s], w[s]], plain images first */
    int32_t h[UAPS_TTA_MAX_SCALES], w[UAPS_TTA_MAX_SCALES];
    float* probs_sum;                            /* [B][C][H][W] or NULL */
    int64_t* mask;                               /* [B][H][W] or NULL */
    float* conf;                                 /* [B][H][W] or NULL; not all three NULL */
    uaps_stream_t stream;
} uaps_tta_fold_call;
int uaps_tta_fold(const uaps_tta_fold_call* call);

/* ---------------------------------------------------------------------------------------------
 * Defect instances and run-length masks: csrc/instances.hip.
 *
 * uaps_label_instances: connected components of a class mask.  mask int64 [B, H, W], any H, W >= 1.  A component is a maximal set of
 *   pixels of one class, different from `background` when has_background == 1 (0: every class forms components), connected under
 *   `connectivity` 4 or 8; touching regions of different classes are different components.  Components with fewer than min_area pixels
 *   are removed.  Within an image the others are numbered 1 .. N_b by the raster index of their first pixel, ascending.
 *     labels int32 [B, H, W]   the number of the pixel's component, 0 for background and removed components; always complete
 *     count  int32 [B]         N_b, whatever max_instances is
 *     table  int64 [B, max_instances, 9]   row k - 1 of image b describes component k:
 *                              class, area, y0, x0, y1, x1 (half-open box), first_pixel (y * W + x), sum0, sum1;
 *                              rows from count[b] on are zero, components numbered above max_instances have no row
 *     sum0 / sum1              over the component's pixels, of q(v) = (int64) rintf(clamp(v, -65536, 65536) * 16777216.0f), q(NaN) = 0,
 *                              v from map0 / map1 (fp32 [B, H, W], either NULL: the column stays 0; map1 needs map0).  Integer sums:
 *                              exact, and the same bits from run to run whatever order the adds arrive in.
 *   Launches: tile-local union-find in LDS, seam merging with agent-scope atomics, flatten + area, a two-level raster-order scan
 *   over the surviving roots, the final pass.  No workgroup waits for another inside a launch.  The call does not synchronise.
 *   workspace: uaps_instances_workspace_bytes(B, H, W) bytes, 256-byte aligned, the call's alone until it has run.
 * Errors (nothing launched): UAPS_EINVAL null struct or mask / labels / count / table / workspace, non-positive dimension,
 *   connectivity outside {4, 8}, min_area < 1, max_instances < 1, has_background outside {0, 1}, map1 without map0, struct_size
 *   below this version's; UAPS_ERANGE H * W >= 2^31, B * H * W * 8 >= 2 GiB, table >= 2 GiB (by dimensions); UAPS_EWORKSPACE.
 *
 * uaps_rle_count / uaps_rle_encode / uaps_rle_decode: the reference's run-length exchange format (utilities/utilities.py:36-63,
 *   mask2rle / make_mask).  The binary plane [mask == classes[c]] of image b is walked in column-major order; a run is a pair
 *   (start, length) with a 1-based start.  Segment j = b * n_classes + c.
 *   uaps_rle_count    mask int64 [B, H, W] -> col_offsets int32 [B * n_classes * W + 1]: the exclusive prefix sums of the number of
 *                     runs that start in column x of segment j, at [j * W + x]; the last word is the total.  So the CSR offsets of the
 *                     segments are col_offsets[j * W], j = 0 .. B * n_classes.
 *   uaps_rle_encode   mask and the col_offsets of uaps_rle_count -> pairs int32 [total, 2].
 *   uaps_rle_decode   pairs int32 [n_runs, 2], offsets int32 [B * n_classes + 1] (device) -> out [B, H, W], int64 or (out_uint8 == 1)
 *                     uint8: zero, then pixels [start - 1, start - 1 + length) of the column-major walk receive classes[c]; later
 *                     classes win where runs overlap (one launch per class, in order).  Runs need not be sorted; what leaves the
 *                     plane is not written.
 * Errors (nothing launched): UAPS_EINVAL null struct or a pointer the call uses, non-positive dimension, negative n_runs, out_uint8
 *   outside {0, 1}, struct_size below this version's; UAPS_ERANGE n_classes outside [1, UAPS_RLE_MAX_CLASSES], H * W >= 2^31, a
 *   tensor of 2 GiB or more (by dimensions), a class outside [0, 255] with out_uint8.
 * ------------------------------------------------------------------------------------------- */
typedef struct uaps_instances_call {
    uint32_t struct_size;
    int32_t B, H, W;
    int32_t connectivity;                        /* 4 or 8 */
    int32_t has_background;                      /* 1: pixels of class `background` form no component */
    int64_t background;
    int32_t min_area, max_instances;
    const int64_t* mask;                         /* [B][H][W] */
    const float* map0;                           /* [B][H][W] or NULL */
    const float* map1;                           /* [B][H][W] or NULL */
    int32_t* labels;                             /* [B][H][W] */
    int32_t* count;                              /* [B] */
    int64_t* table;                              /* [B][max_instances][9] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_instances_call;
int uaps_instances_workspace_bytes(int B, int H, int W, size_t* bytes);
int uaps_label_instances(const uaps_instances_call* call);

#define UAPS_RLE_MAX_CLASSES 8
typedef struct uaps_rle_call {
    uint32_t struct_size;
    int32_t B, H, W, n_classes;
    int64_t classes[UAPS_RLE_MAX_CLASSES];
    const int64_t* mask;                         /* count, encode: [B][H][W] */
    int32_t* col_offsets;                        /* count writes, encode reads: [B * n_classes * W + 1] */
    int32_t* pairs;                              /* encode writes, decode reads: [runs][2] */
    const int32_t* offsets;                      /* decode: [B * n_classes + 1] */
    int64_t n_runs;                              /* decode: rows of pairs */
    void* out;                                   /* decode: [B][H][W] int64, or uint8 with out_uint8 == 1 */
    int32_t out_uint8;
    uaps_stream_t stream;
} uaps_rle_call;
int uaps_rle_count(const uaps_rle_call* call);
int uaps_rle_encode(const uaps_rle_call* call);
int uaps_rle_decode(const uaps_rle_call* call);

/* ---------------------------------------------------------------------------------------------
 * Mask clean-up morphology: csrc/morph.hip.
 *
 * uaps_morphology: a chain of n_steps steps (op, footprint, radius), applied in order, on a label map.  mask and out int64
 *   [B, H, W], out != mask.
 *   Footprint of radius r: the offsets (dy, dx) with |dy| <= r and |dx| <= w(dy); square w = r, cross (the L1 ball) w = r - |dy|,
 *   disk w = floor(sqrt(r * r - dy * dy)) formed in integers.
 *   Border: erosion takes what lies outside the image as foreground, dilation as background (scipy's border_value 1 and 0), so an
 *   opening does not eat a defect that touches the edge; opening stays anti-extensive, closing extensive.
 *   One step: for every selected class c (classes[0 .. n_classes), any order), on the plane P_c = (mask == c) alone,
 *     R_c = P_c - S (erode), P_c + S (dilate), (P_c - S) + S (open), (P_c + S) - S (close), P_c \ (P_c - S) (boundary).
 *   Then per pixel p of value m: m selected and p in R_m: stays m.  Otherwise m neither `background` nor selected (an ignore label,
 *   a class the call does not name): stays m -- such pixels are obstacles, never claimed.  Otherwise (background, or just removed):
 *   the smallest selected c with p in R_c, `background` if there is none.  The next step sees that map.
 *   One launch for the whole chain; a workgroup holds a band of rows (of at most 512 columns) and a halo of `reach` rows -- the sum
 *   of r over erode / dilate / boundary steps and of 2 r over open / close steps -- as bit planes in at most 64 KiB of LDS.
 *   band_rows 0: the band height uaps_morph_band_rows reports; > 0: that height (every height gives the same bits).  No workspace,
 *   no atomics, no synchronisation with the host.
 * uaps_morph_band_rows (host only): the band height 0 resolves to for n_planes = n_classes + 1 bit planes (the selected classes and
 *   the obstacle plane).  UAPS_EINVAL rows == NULL, a non-positive dimension, n_planes outside [2, 9], reach < 1; UAPS_ERANGE as below.
 * Errors (nothing launched): UAPS_EINVAL null struct, mask or out, out == mask, non-positive dimension, n_steps outside [1, 8], an
 *   unknown op or footprint, n_classes outside [1, 8], a duplicate class or one equal to `background`, negative band_rows, struct_size
 *   below this version's; UAPS_ERANGE a radius outside [1, 15], reach > 64, H or W above 4096, B * H * W * 8 >= 2 GiB, a forced
 *   band_rows whose planes do not fit.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_MORPH_ERODE 0
#define UAPS_MORPH_DILATE 1
#define UAPS_MORPH_OPEN 2
#define UAPS_MORPH_CLOSE 3
#define UAPS_MORPH_BOUNDARY 4
#define UAPS_MORPH_SQUARE 0
#define UAPS_MORPH_CROSS 1
#define UAPS_MORPH_DISK 2
#define UAPS_MORPH_MAX_STEPS 8
#define UAPS_MORPH_MAX_CLASSES 8
typedef struct uaps_morph_call {
    size_t struct_size;
    int32_t B, H, W;
    int32_t n_steps;
    int32_t op[UAPS_MORPH_MAX_STEPS], footprint[UAPS_MORPH_MAX_STEPS], radius[UAPS_MORPH_MAX_STEPS];
    int32_t n_classes;
    int32_t classes[UAPS_MORPH_MAX_CLASSES];
    int32_t background;
    int32_t band_rows;                           /* 0: chosen by the library; > 0: forced (tests) */
    const int64_t* mask;                         /* [B][H][W] */
    int64_t* out;                                /* [B][H][W] */
    uaps_stream_t stream;
} uaps_morph_call;
int uaps_morphology(const uaps_morph_call* call);
int uaps_morph_band_rows(int H, int W, int n_planes, int reach, int* rows);

/* ---------------------------------------------------------------------------------------------
 * Component clean-up of a label map: csrc/components.hip (the labelling passes: csrc/cc_common.hpp, shared with csrc/instances.hip).
 *
 * uaps_components: a chain of n_steps steps (kind, n), applied in order, on a label map.  mask and out int64 [B, H, W], out != mask,
 *   any H, W >= 1.  A component is a maximal set of equal-valued pixels connected under `connectivity` (4 or 8), as
 *   uaps_label_instances defines it.  classes[0 .. n_classes) are the selected classes, in any order.
 *     UAPS_COMP_AREA_OPEN, n >= 1   every component of a selected class with fewer than n pixels becomes `background` (area >= n stays:
 *                                   the keep rule of uaps_label_instances' min_area).
 *     UAPS_COMP_CLEAR_BORDER        every component of a selected class with a pixel in row 0, row H - 1, column 0 or column W - 1
 *                                   becomes `background`; n is not read.
 *     UAPS_COMP_FILL_HOLES, n >= 1  for every selected class c, a hole of c is a connected component of the complement of
 *                                   P_c = (mask == c) -- background, other classes and ignore labels alike -- that has no pixel on the
 *                                   image border, connected under the COMPLEMENTARY connectivity (4 where connectivity == 8, 8 where
 *                                   it is 4).  A hole of at most n pixels (all of its pixels count, not only the background ones) is
 *                                   filled; n = UAPS_COMP_ALL: every hole.  All planes are evaluated on the step's input; only pixels
 *                                   whose value is `background` are rewritten, and one that lies in a filled hole of several classes
 *                                   goes to the smallest of them.  Every other pixel inside a hole stays and is never claimed.
 *   Area opening and clear border only ever write `background`, and only over pixels of selected classes.
 *   Launches per step: tile-local union-find in LDS, seam merging with agent-scope atomics, flatten + area + border flag, one apply
 *   pass that writes the step's map once (hole filling labels B * n_classes virtual planes read from the map; no one-hot tensor).
 *   Integer atomics only: the same bits from run to run.  No workgroup waits for another inside a launch.  The call does not
 *   synchronise; the area and flag words are zeroed inside the call for every step.
 *   workspace: uaps_components_workspace_bytes(B, H, W, n_planes) bytes, 256-byte aligned, the call's alone until it has run;
 *   n_planes = n_classes for a chain with a UAPS_COMP_FILL_HOLES step, 1 for a chain without.
 * Errors (nothing launched): UAPS_EINVAL null struct, mask, out or workspace, out == mask, non-positive dimension, n_steps outside
 *   [1, 8], an unknown kind, n < 1 in an area-open or hole-filling step, n_classes outside [1, 8], a duplicate class or one equal to
 *   `background`, connectivity outside {4, 8}, struct_size below this version's (uaps_components_workspace_bytes: bytes == NULL,
 *   non-positive dimension, n_classes outside [1, 8]); UAPS_ERANGE H * W >= 2^31, B * H * W * 8 >= 2 GiB, a workspace of 2 GiB or
 *   more (by dimensions); UAPS_EWORKSPACE a workspace smaller than that or not 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_COMP_AREA_OPEN 0
#define UAPS_COMP_CLEAR_BORDER 1
#define UAPS_COMP_FILL_HOLES 2
#define UAPS_COMP_MAX_STEPS 8
#define UAPS_COMP_MAX_CLASSES 8
#define UAPS_COMP_ALL 2147483647                 /* n of a hole-filling step: every hole, whatever its area */
typedef struct uaps_components_call {
    size_t struct_size;
    int32_t B, H, W;
    int32_t n_steps;
    int32_t kind[UAPS_COMP_MAX_STEPS], n[UAPS_COMP_MAX_STEPS];
    int32_t n_classes;
    int32_t classes[UAPS_COMP_MAX_CLASSES];
    int32_t background;
    int32_t connectivity;                        /* 4 or 8: of the defects; holes take the other one */
    const int64_t* mask;                         /* [B][H][W] */
    int64_t* out;                                /* [B][H][W] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_components_call;
int uaps_components_workspace_bytes(int B, int H, int W, int n_classes, size_t* bytes);
int uaps_components(const uaps_components_call* call);

/* ---------------------------------------------------------------------------------------------
 * Hysteresis thresholding and binary reconstruction: csrc/hysteresis.hip (the labelling passes: csrc/cc_common.hpp).
 *
 * uaps_hysteresis: the seeded components of a score map, or of a label map and a marker map.  out int64 [B, H, W], any H, W >= 1.
 *   classes[0 .. n_classes) are the selected classes, strictly ascending, none equal to `background`.
 *   Score form (scores != NULL; mask and markers NULL): scores fp32 [B, C, H, W], 1 <= C <= UAPS_MAX_CLASSES.  from_logits: the
 *     softmax over all C channels is formed in the kernel (C == 1: the sigmoid 1 / (1 + exp(-z))).  classes lie in [0, C); C == 1:
 *     the one channel is the score of class 1 and classes = {1}.  A pixel's class c* is the arg-max of its scores over the SELECTED
 *     classes alone (the lowest class among equal scores); it is a CANDIDATE of c* iff s[c*] >= low[k*] and a SEED iff
 *     s[c*] >= high[k*], k* the place of c* in `classes`, compared in fp32.  A pixel with a NaN among its selected scores is neither.
 *     Components are maximal sets of candidates of one class connected under `connectivity` (4 or 8).  A component survives iff it
 *     holds a seed and has at least min_area pixels.  out: the class on surviving pixels, `background` elsewhere.
 *   Marker form (scores == NULL): mask int64 [B, H, W], markers uint8 [B, H, W] (non-zero: seed), out != mask; C, from_logits, low and
 *     high are not read.  A component of a selected class of `mask` survives iff one of its own pixels has a non-zero marker and it
 *     has at least min_area pixels; dropped pixels become `background`; every other value (ignore labels, unselected classes)
 *     passes through untouched, and a marker on such a pixel marks nothing.
 *   Launches: a classify pass writes an int64 code map into the workspace (class + 1 in the low word, 0: forms nothing; bit 32: seed);
 *   tile-local union-find in LDS and seam merging with agent-scope atomics on that map (one labelling for all classes); flatten +
 *   area with the seed raising bit 31 of the root's area word; one apply pass that writes `out` once.  Integer atomics only: the same
 *   bits from run to run.  No workgroup waits for another inside a launch.  The call does not synchronise; the area and flag words
 *   are zeroed inside the call.
 *   workspace: uaps_hysteresis_workspace_bytes(B, H, W) bytes (16 a pixel), 256-byte aligned, the call's alone until it has run.
 * Errors (nothing launched): UAPS_EINVAL null struct, out or workspace, neither or both forms' operands, out == mask, non-positive
 *   dimension, n_classes outside [1, 8], classes not strictly ascending, negative or equal to `background`, a class outside [0, C)
 *   (C == 1: other than 1), from_logits outside {0, 1}, low > high or a NaN threshold, connectivity outside {4, 8}, min_area < 1,
 *   struct_size below this version's (uaps_hysteresis_workspace_bytes: bytes == NULL, non-positive dimension); UAPS_ERANGE C outside
 *   [1, UAPS_MAX_CLASSES], H * W >= 2^31, B * H * W * 8 >= 2 GiB, scores or the workspace of 2 GiB or more (by dimensions);
 *   UAPS_EWORKSPACE a workspace smaller than that or not 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_HYST_MAX_CLASSES 8
typedef struct uaps_hysteresis_call {
    size_t struct_size;
    int32_t B, C, H, W;                          /* C: channels of scores (not read in the marker form) */
    int32_t from_logits;
    int32_t n_classes;
    int32_t classes[UAPS_HYST_MAX_CLASSES];      /* strictly ascending */
    float low[UAPS_HYST_MAX_CLASSES], high[UAPS_HYST_MAX_CLASSES];   /* per selected class, low <= high; +-inf allowed */
    int32_t background;
    int32_t connectivity;                        /* 4 or 8 */
    int32_t min_area;                            /* >= 1 */
    const float* scores;                         /* [B][C][H][W], or NULL: the marker form */
    const int64_t* mask;                         /* [B][H][W]  (marker form) */
    const uint8_t* markers;                      /* [B][H][W]  (marker form) */
    int64_t* out;                                /* [B][H][W] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_hysteresis_call;
int uaps_hysteresis_workspace_bytes(int B, int H, int W, size_t* bytes);
int uaps_hysteresis(const uaps_hysteresis_call* call);

/* ---------------------------------------------------------------------------------------------
 * Splitting of touching defects: csrc/split.hip (the labelling passes: csrc/cc_common.hpp; numbering and table: csrc/instances.hip).
 *
 * uaps_split_instances: the components of uaps_label_instances (source_labels int32 [B, H, W], source_table int64
 *   [B, source_rows, 9]) cut into the geodesic zones of influence of their MARKERS.  H, W <= UAPS_SPLIT_MAX_EXTENT.
 *   Marker pixels: a pixel with source label > 0 and, distance form (distance != NULL, markers NULL), distance[pixel] >= d2 --
 *     distance int32 [B, H, W], usually uaps_edt_sq of the source labels -- or, marker form (markers != NULL, distance NULL),
 *     markers[pixel] != 0 (uint8 [B, H, W]; d2 is not read).
 *   Markers: the maximal sets of marker pixels of ONE source label under `connectivity` (4 or 8) with at least min_marker_area
 *     pixels.  A marker's id is the image-local raster index of its first pixel, plus 1.
 *   Owners: round 0, a pixel of a marker owns that marker's id, every other pixel 0.  One synchronous round: every pixel with source
 *     label > 0 and owner 0 takes the smallest non-zero owner among its neighbours (under `connectivity`) of the same source label,
 *     all pixels reading the state of the round's start.  The result is the state after min(max_iters, rounds until nothing
 *     changes) rounds; converged[b] (uint8 [B]) = 1 iff image b is at the fixed point.
 *   Pieces: maximal connected sets (under `connectivity`) of equal (source label, owner), numbered and tabulated exactly as
 *     uaps_label_instances does it: labels int32 [B, H, W], count int32 [B] (complete whatever max_instances is), table int64
 *     [B, max_instances, 9] with the same columns, pieces below min_area pixels removed, map0 / map1 summed as there.  The class
 *     column is source_table's class of the piece's source label, -1 for a source label above source_rows.
 *     parent int32 [B, max_instances]: the source label of piece k, 0 in rows without a piece.  pieces int32 [B, source_rows]: how
 *     many rows of `parent` name each source label.
 *   Launches: a classify pass (the marker code map), the three labelling passes of cc_common.hpp on it, an init pass (the owner plane),
 *   ceil(max_iters / S) growth launches of S rounds each on tiles staged in LDS -- S = sub_iters, 0: the default; a launch returns
 *   at once once its image stopped changing -- a check pass, a code pass, the seven launches of uaps_label_instances on the code map
 *   (label << 32) | owner and one fix-up pass over the table rows.  Integer atomics only: the same bits from run to run and for every
 *   sub_iters, band_rows and tile_cols (0: the plan's; uaps_split_band_rows answers what that is).  The call does not synchronise;
 *   everything the workspace carries is written inside the call before it is read.
 *   workspace: uaps_split_workspace_bytes(B, H, W) bytes (about 24 a pixel), 256-byte aligned, the call's alone until it has run.
 * Errors (nothing launched): UAPS_EINVAL null struct, a null operand other than map0 / map1, both or neither of distance and
 *   markers, map1 without map0, non-positive dimension, connectivity outside {4, 8}, min_area, min_marker_area, max_instances or
 *   source_rows < 1, d2 < 0, max_iters outside [1, UAPS_SPLIT_MAX_ITERS], sub_iters outside [0, UAPS_SPLIT_MAX_SUB_ITERS], negative
 *   band_rows or tile_cols, struct_size below this version's; UAPS_ERANGE H or W above UAPS_SPLIT_MAX_EXTENT, B * H * W * 8 >= 2 GiB,
 *   a table or the workspace of 2 GiB or more (by dimensions), a forced tile that does not fit 64 KiB of LDS with its halo;
 *   UAPS_EWORKSPACE a workspace smaller than uaps_split_workspace_bytes or not 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_SPLIT_MAX_EXTENT 4096
#define UAPS_SPLIT_MAX_ITERS 65536
#define UAPS_SPLIT_MAX_SUB_ITERS 16
typedef struct uaps_split_call {
    size_t struct_size;
    int32_t B, H, W;
    int32_t connectivity;                        /* 4 or 8: the one the source was labelled with */
    int32_t d2;                                  /* distance form: >= 0 */
    int32_t min_marker_area;                     /* >= 1 */
    int32_t max_iters;                           /* 1 .. UAPS_SPLIT_MAX_ITERS */
    int32_t sub_iters;                           /* rounds a launch; 0: the default */
    int32_t band_rows, tile_cols;                /* owned rows and columns of a tile; 0: the plan's */
    int32_t min_area;                            /* >= 1, of the pieces */
    int32_t max_instances;                       /* rows of table and parent */
    int32_t source_rows;                         /* rows of source_table and pieces */
    const int32_t* source_labels;                /* [B][H][W] */
    const int64_t* source_table;                 /* [B][source_rows][9] */
    const int32_t* distance;                     /* [B][H][W], or NULL: the marker form */
    const uint8_t* markers;                      /* [B][H][W], or NULL: the distance form */
    const float* map0;                           /* [B][H][W] or NULL */
    const float* map1;
    int32_t* labels;                             /* [B][H][W] */
    int32_t* count;                              /* [B] */
    int64_t* table;                              /* [B][max_instances][9] */
    int32_t* parent;                             /* [B][max_instances] */
    int32_t* pieces;                             /* [B][source_rows] */
    uint8_t* converged;                          /* [B] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_split_call;
int uaps_split_workspace_bytes(int B, int H, int W, size_t* bytes);
int uaps_split_band_rows(int H, int W, int sub_iters, int* rows, int* cols);
int uaps_split_instances(const uaps_split_call* call);

/* ---------------------------------------------------------------------------------------------
 * Defect shape descriptors: csrc/shapes.hip.
 *
 * uaps_shape_descriptors: raw moments, Gray's bit-quad counts and the statistics of an optional plane, per component of the
 *   `labels` of uaps_label_instances.  labels int32 [B, H, W]: 0 = no component, k >= 1 = component k of that image.
 *     table int64 [B, max_instances, 11]   row k - 1 of image b describes the pixels of image b whose label is k, 1 <= k <= max_instances:
 *       0..4  sy, sx, syy, sxy, sxx   the sums of y, x, y * y, x * y, x * x over the component's pixels (row y, column x, absolute)
 *       5..8  q1, q2, q3, qd          bit-quad counts over the (H + 1) x (W + 1) windows {(i-1, j-1), (i-1, j), (i, j-1), (i, j)},
 *                                     0 <= i <= H, 0 <= j <= W, pixels outside the image belonging to no component: with n the
 *                                     number of window pixels labelled k, n = 1 adds to q1, n = 2 to q2 (the two share an edge) or qd
 *                                     (they are diagonal), n = 3 to q3, n = 4 to nothing
 *       9..10 pmax, psum              the maximum and the sum of max(plane, 0) over the component; plane int32 [B, H, W], or NULL:
 *                                     both stay 0
 *     A label <= 0 or above max_instances has no row, and counts as "not k" for every other component.  Rows without a component
 *     are zero: the call zeroes the whole table itself.  All columns are exact integers below 2^59.
 *   One zeroing launch and one pass over labels (and plane).  A wave owns 64 consecutive pixels of a row and reads rows y - 1, y,
 *   y + 1; every (window, component) pair is counted by the first pixel of the window, in raster order, that carries the label; all
 *   columns are reduced over runs of equal labels along the row.  Up to UAPS_SHAPE_LDS_ROWS rows a workgroup (rows of one image)
 *   adds its runs into a copy of the image's table in LDS and sends the non-zero words with 64-bit atomics; above that the runs' first
 *   lanes send them directly.  Integer atomics only: the same bits from run to run and from either form.  No workspace; the call
 *   does not synchronise.
 * Errors (nothing launched): UAPS_EINVAL null struct, labels or table, table == labels, non-positive dimension, max_instances < 1,
 *   struct_size below this version's; UAPS_ERANGE H or W above UAPS_SHAPE_MAX_EXTENT, H * W >= 2^31, B * H * W * 8 >= 2 GiB, a
 *   table of 2 GiB or more (by dimensions).
 * ------------------------------------------------------------------------------------------- */
#define UAPS_SHAPE_COLUMNS 11
#define UAPS_SHAPE_MAX_EXTENT 16384
#define UAPS_SHAPE_LDS_ROWS 256                  /* max_instances up to which a workgroup combines its runs in LDS */
typedef struct uaps_shape_call {
    uint32_t struct_size;
    int32_t B, H, W, max_instances;
    const int32_t* labels;                       /* [B][H][W] */
    const int32_t* plane;                        /* [B][H][W] or NULL */
    int64_t* table;                              /* [B][max_instances][11], written whole */
    uaps_stream_t stream;
} uaps_shape_call;
int uaps_shape_descriptors(const uaps_shape_call* call);

/* ---------------------------------------------------------------------------------------------
 * Defect skeletons: csrc/skeleton.hip.
 *
 * uaps_skeletonize: Guo and Hall's two-subiteration parallel thinning (CACM 32(3), 1989, algorithm A1) of a label map.  mask and
 *   out int64 [B, H, W], out != mask.  Every selected class c (classes[0 .. n_classes), any order) is thinned on its own plane
 *   P_c = (mask == c), 8-connected, everything outside the image background; a selected pixel that thinning removes becomes
 *   `background`, every other value passes through untouched and is never claimed.
 *   With the neighbours P2..P9 = N, NE, E, SE, S, SW, W, NW of a pixel,
 *     C  = [!P2 & (P3 | P4)] + [!P4 & (P5 | P6)] + [!P6 & (P7 | P8)] + [!P8 & (P9 | P2)],
 *     N1 = (P9 | P2) + (P3 | P4) + (P5 | P6) + (P7 | P8),  N2 = (P2 | P3) + (P4 | P5) + (P6 | P7) + (P8 | P9),  N = min(N1, N2),
 *   a foreground pixel is deleted in a sub-iteration iff C == 1, 2 <= N <= 3 and (P2 | P3 | !P5) & P4 == 0 in the first
 *   sub-iteration of an iteration, (P6 | P7 | !P9) & P8 == 0 in the second.  Every sub-iteration is a pure function of the
 *   previous plane; an iteration is the two sub-iterations in that order.
 *   out is the map after exactly min(max_iters, iterations to the fixed point) iterations.  converged uint8 [B]: 1 exactly where
 *   the returned image is a fixed point for every selected class (one more iteration would delete nothing), else 0.
 *   Launches: one pass packs the class planes into 64-bit words (a wave64 ballot of mask == c is the word), ceil(2 * max_iters / S)
 *   thinning launches of S sub-iterations each (the last one the rest) on the packed planes, ping-pong between the two halves of
 *   the workspace, one pass that tests the fixed point and one that writes the int64 map: fixed by the arguments.  A thinning
 *   workgroup stages a band of rows x at most 512 columns of one plane in LDS with S halo rows and one halo word left and right;
 *   the rule is evaluated bit-sliced on the words, without a table.  A per-image word records the last launch that removed
 *   anything; a launch that finds the launch before it removed nothing from its image returns at once (both halves of the
 *   workspace then hold the same planes).  Integers only, no atomics: the same bits from run to run, for every band height and S.
 *   sub_iters 0: the S the library chooses; else an even value in [2, 64].  band_rows 0: the band height uaps_skeleton_band_rows
 *   reports; > 0: that height.
 *   workspace: uaps_skeleton_workspace_bytes(B, H, W, n_classes) bytes, 256-byte aligned, the call's alone until it has run; it
 *   need not be zeroed.
 * uaps_skeleton_band_rows (host only): the band height 0 resolves to for n_planes = n_classes + 1 and S sub-iterations a launch
 *   (S 0: the chosen one).
 * Errors (nothing launched): UAPS_EINVAL null struct, mask, out, converged or workspace, out == mask, non-positive dimension,
 *   n_classes outside [1, 8], a duplicate class or one equal to `background`, max_iters outside [1, 2048], sub_iters odd or outside
 *   {0} + [2, 64], negative band_rows, struct_size below this version's (the queries: a NULL result pointer, non-positive
 *   dimension, n_classes outside [1, 8], n_planes outside [2, 9], S likewise); UAPS_ERANGE H or W above 4096, B * H * W * 8 >=
 *   2 GiB, a workspace of 2 GiB or more (by dimensions), a forced band_rows whose planes do not fit 64 KiB of LDS;
 *   UAPS_EWORKSPACE a workspace smaller than that or not 256-byte aligned.
 *
 * uaps_skeleton_stats: per defect of uaps_label_instances' `labels`, the counts that give a skeleton's length, its ends and its
 *   branch points.  labels int32 [B, H, W], skel int64 [B, H, W] (the `out` of uaps_skeletonize on the mask the labels were formed
 *   from).  A pixel p is a skeleton pixel of defect k iff labels[p] == k, 1 <= k <= max_instances, and skel[p] is one of
 *   classes[0 .. n_classes).  Two skeleton pixels are linked iff they are 8-adjacent and belong to the same defect.
 *     table int64 [B, max_instances, 7], row k - 1:
 *       0 n_skel    skeleton pixels of the defect
 *       1 n_orth    links between edge-adjacent skeleton pixels, each counted once
 *       2 n_diag    links between diagonally adjacent skeleton pixels where neither of the two pixels edge-adjacent to both is a
 *                   skeleton pixel of the same defect, each counted once
 *       3 n_end     skeleton pixels with exactly one linked neighbour
 *       4 n_branch  skeleton pixels whose cyclic sequence N, NE, E, SE, S, SW, W, NW of "is linked" has at least three 0 -> 1 steps
 *       5 d2max, 6 d2sum   the maximum and the sum of max(plane, 0) over the skeleton pixels; plane int32 [B, H, W], or NULL: 0
 *     A label <= 0 or above max_instances has no row and counts as "not the same defect".  Rows without a component are zero: the
 *     call zeroes the whole table itself.
 *   One zeroing launch and one pass: a wave owns 64 consecutive pixels of a row, reads rows y - 1, y, y + 1 and takes the side
 *   neighbours from shuffles; a link is counted by its raster-first end (E, SW, S, SE); values are reduced over runs of equal
 *   labels and flushed as uaps_shape_descriptors does (LDS copy of the table up to UAPS_SHAPE_LDS_ROWS rows, directly above it).
 *   Integer atomics on non-negative values only.  No workspace; the call does not synchronise.
 * Errors (nothing launched): UAPS_EINVAL null struct, labels, skel or table, non-positive dimension, max_instances < 1, n_classes
 *   outside [1, 8], struct_size below this version's; UAPS_ERANGE as uaps_shape_descriptors (the table has 7 columns).
 * ------------------------------------------------------------------------------------------- */
#define UAPS_SKEL_MAX_CLASSES 8
#define UAPS_SKEL_MAX_ITERS 2048
#define UAPS_SKEL_MAX_SUB_ITERS 64
#define UAPS_SKEL_MAX_EXTENT 4096
#define UAPS_SKEL_COLUMNS 7
typedef struct uaps_skeleton_call {
    size_t struct_size;
    int32_t B, H, W;
    int32_t n_classes;
    int32_t classes[UAPS_SKEL_MAX_CLASSES];
    int32_t background;
    int32_t max_iters;
    int32_t sub_iters;                           /* 0: chosen by the library; else even, 2..64 (tests) */
    int32_t band_rows;                           /* 0: chosen by the library; > 0: forced (tests) */
    const int64_t* mask;                         /* [B][H][W] */
    int64_t* out;                                /* [B][H][W] */
    uint8_t* converged;                          /* [B] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_skeleton_call;
int uaps_skeleton_workspace_bytes(int B, int H, int W, int n_classes, size_t* bytes);
int uaps_skeleton_band_rows(int H, int W, int n_planes, int S, int* rows);
int uaps_skeletonize(const uaps_skeleton_call* call);

typedef struct uaps_skeleton_stats_call {
    uint32_t struct_size;
    int32_t B, H, W, max_instances;
    int32_t n_classes;
    int32_t classes[UAPS_SKEL_MAX_CLASSES];
    const int32_t* labels;                       /* [B][H][W] */
    const int64_t* skel;                         /* [B][H][W] */
    const int32_t* plane;                        /* [B][H][W] or NULL */
    int64_t* table;                              /* [B][max_instances][7], written whole */
    uaps_stream_t stream;
} uaps_skeleton_stats_call;
int uaps_skeleton_stats(const uaps_skeleton_stats_call* call);

/* ---------------------------------------------------------------------------------------------
 * Tiled (sliding-window) full-resolution inference: csrc/tiled.hip.  An image of any size is cut into overlapping tiles of the size
 * the network runs at, the network runs on the tiles, and the tiles' probability maps are blended under a separable window.
 *
 * Geometry, per axis, with image extent n, tile extent t >= 1, overlap o, 0 <= o <= t / 2 (integer division), stride s = t - o:
 *   n <= t   one tile at origin 0; its positions i >= n are mirror padding without repeating the edge: the source of position i is
 *            m(i, n) = 0 when n == 1, else j = i mod 2 (n - 1), m = j when j < n, else 2 (n - 1) - j (any amount of padding).
 *   n >  t   origins 0, s, 2 s, ... while < n - t, then a last origin n - t: the last tile is clamped into the image and overlaps its
 *            neighbour by more.  No tile leaves the image, nothing is padded.
 *   With o <= t / 2 a pixel lies in at most 3 tiles per axis (two regular ones and the clamped one), 9 in all.
 *   Tiles are numbered g = b * T + iy * nx + ix, image-major, T = ny * nx.
 * uaps_tile_origins (host only, launches nothing): *count = the number of tiles of one axis; origins, when not NULL, receives the first
 *   min(*count, cap) origins in ascending order.  UAPS_EINVAL count == NULL, n < 1, tile < 1, overlap < 0, cap < 0; UAPS_ERANGE
 *   overlap > tile / 2.
 *
 * uaps_tile_cut: x [B, Cin, H, W] -> out [g1 - g0, Cin, th, tw], the tiles g0 <= g < g1 of the numbering above; a pure copy (with the
 *   mirrored index where an extent is below the tile's), bit-exact.  One launch per chunk of tiles: the caller bounds the forward's batch.
 * uaps_tile_fold: the output side in one launch, gather form.  The tiles' logits [., C, th, tw] are read where the forwards left them:
 *   logits[k] is the base of chunk k, which holds tiles [k * tiles_per_chunk, min((k + 1) * tiles_per_chunk, B * T)); n_chunks is
 *   ceil(B * T / tiles_per_chunk) exactly.  A lane owns an output pixel (or four consecutive ones), finds the covering tiles from the
 *   origin formula, and visits them in ascending (iy, ix) order: softmax over the C logits at the pixel, times wy[r] * wx[c] (r, c =
 *   the pixel's position in the tile), added to C register accumulators and to the weight sum; at the end everything is divided by the
 *   weight sum.  Written, whichever are not NULL:
 *     probs [B, C, H, W] the weighted mean of the tiles' softmax (sums to 1);  mask [B, H, W] int64 its arg-max, the lowest index among
 *     equal values;  conf [B, H, W] its largest value.
 *   maps[m][k] (m < n_maps <= UAPS_TILE_MAX_MAPS): chunk k of a per-tile scalar map [., th, tw], blended by the same weights into
 *     map_out[m] [B, H, W].  C == 0 with probs, mask and conf NULL and n_maps >= 1 blends maps alone.
 *   wy [th], wx [tw]: fp32, device memory, every entry finite and > 0.  Other values give undefined values in the outputs, never an
 *   access out of bounds.  Mirror padding of a tile is never read.  No LDS, no atomics, a fixed order: two runs give the same bits, and
 *   so do two chunkings of the same tiles.  With W % 4 == 0 and 16-byte aligned outputs a lane owns four consecutive pixels and stores
 *   16 bytes; otherwise one pixel -- the same arithmetic per pixel either way.
 * Both structs are size-versioned like the test-time augmentation's.  The calls do not synchronise.
 * Errors (nothing launched): UAPS_EINVAL null struct, struct_size below this version's, x / out / wy / wx NULL, no output at all, a
 *   logits (C > 0) or maps chunk pointer or a map_out NULL below its count, non-positive dimension, negative overlap / C / n_maps,
 *   C == 0 with probs, mask or conf, C > 0 with none of them, n_chunks != ceil(B * T / tiles_per_chunk), g0 / g1 outside 0 <= g0 < g1 <= B * T;
 *   UAPS_ERANGE overlap > tile / 2, C == 1 (one-channel sigmoid heads have no form here) or C > UAPS_MAX_CLASSES, n_chunks >
 *   UAPS_TILE_MAX_CHUNKS, n_maps > UAPS_TILE_MAX_MAPS, a tensor of 2 GiB or more (by dimensions; of the outputs only those that are
 *   not NULL count).
 * ------------------------------------------------------------------------------------------- */
#define UAPS_TILE_MAX_CHUNKS 32
#define UAPS_TILE_MAX_MAPS 2
int uaps_tile_origins(int n, int tile, int overlap, int* count, int* origins, int cap);

typedef struct uaps_tile_cut_call {
    uint32_t struct_size;
    int32_t B, Cin, H, W;
    int32_t th, tw, oy, ox;                      /* tile extents and overlaps along y and x */
    int32_t g0, g1;                              /* the tiles this launch writes */
    const float* x;                              /* [B][Cin][H][W] */
    float* out;                                  /* [g1 - g0][Cin][th][tw] */
    uaps_stream_t stream;
} uaps_tile_cut_call;
int uaps_tile_cut(const uaps_tile_cut_call* call);

typedef struct uaps_tile_fold_call {
    uint32_t struct_size;
    int32_t B, C, H, W;
    int32_t th, tw, oy, ox;
    int32_t n_chunks, tiles_per_chunk, n_maps;
    const float* logits[UAPS_TILE_MAX_CHUNKS];   /* device, chunk k: [tiles of the chunk][C][th][tw] */
    const float* maps[UAPS_TILE_MAX_MAPS][UAPS_TILE_MAX_CHUNKS];    /* device, chunk k of map m: [tiles of the chunk][th][tw] */
    const float* wy;                             /* [th] */
    const float* wx;                             /* [tw] */
    float* probs;                                /* [B][C][H][W] or NULL */
    int64_t* mask;                               /* [B][H][W] or NULL */
    float* conf;                                 /* [B][H][W] or NULL */
    float* map_out[UAPS_TILE_MAX_MAPS];          /* [B][H][W] each */
    uaps_stream_t stream;
} uaps_tile_fold_call;
int uaps_tile_fold(const uaps_tile_fold_call* call);

/* ---------------------------------------------------------------------------------------------
 * Boundary metrics: csrc/surface.hip.  An exact squared Euclidean distance transform (separable, integers only) and, on top of it,
 * the directed surface distances between two label maps reduced to one int64 row per (image, class).  2-D maps, isotropic pixels,
 * 1 <= H, W <= UAPS_SURFACE_MAX_EXTENT.  Every quantity is an integer: results are exact and the same bits from run to run.
 *
 * Labels travel as `*_dtype` = UAPS_LABEL_U8 / _I32 / _I64 (the element type of the array behind the pointer).
 *
 * uaps_edt_sq: out int32 [B, H, W] = the squared distance of every pixel to the nearest pixel whose mask value is 0 (0 at such
 *   pixels; scipy.ndimage.distance_transform_edt(mask) squared); UAPS_EDT_NO_FEATURE everywhere in an image without a zero pixel.
 *   Two launches: a column sweep (one lane per column, down and up) that writes the distance along the column as uint16, and a row
 *   pass that stages one row of its squares in LDS, where every lane scans outwards from its pixel until dx^2 reaches its best value.
 *   workspace: uaps_edt_workspace_bytes(B, H, W) bytes, 256-byte aligned, the call's alone until it has run.
 *
 * uaps_surface_distances: pred and target are label maps [B, H, W]; a value outside [0, C) belongs to no class.  With pred_scores
 *   (fp32 [B, C, H, W]) instead of pred, the prediction is its arg-max over the classes, the lowest index among equal scores.
 *   The surface of class c in a map m: m == c and one of the four neighbours is != c or outside the image.  For every surface pixel
 *   of the prediction d2_pg = the smallest dy^2 + dx^2 to a surface pixel of the target, d2_gp likewise the other way round.
 *     table int64 [B, C, UAPS_SURFACE_COLUMNS]: n_pred, n_gt, max_pg, max_gp, sum16_pg, sum16_gp, within_pg, within_gp, rank_lo,
 *       rank_hi, q_lo, q_hi.  sum16 = sum of floor(2^16 sqrt(d2)) (the integer square root of d2 << 32); within = the number of
 *       surface pixels with d2 <= tol_d2 (0 with has_tolerance == 0); with N = n_pred + n_gt and h = (double)(N - 1) * percentile_frac,
 *       rank_lo = floor(h), rank_hi = min(rank_lo + 1, N - 1), and q_lo / q_hi the squared distances of those ranks among the N
 *       pooled values in ascending order.  A pair with n_pred == 0 or n_gt == 0 has zeros in every column after n_gt.
 *   Launches: [arg-max,] the column sweep for both sides and all classes from one read of each label map (surface membership is
 *   decided on the fly, no surface mask is written), the row pass (only lanes on a surface pixel scan; counts, maxima and sums go
 *   through a workgroup reduction and 64-bit integer atomics), the ranks, then three histogram passes (9 + 8 + 8 bits, LDS histograms
 *   flushed with integer atomics, many workgroups per plane) each followed by the choice of the bin.  No float atomics; the call does
 *   not synchronise.
 *   workspace: uaps_surface_workspace_bytes(B, C, H, W) bytes, 256-byte aligned, the call's alone until it has run.
 * Both structs are size-versioned (fields are only ever appended; a larger struct_size is accepted and what it appends is not read).
 * Errors (nothing launched): UAPS_EINVAL null struct or a pointer the call uses, both or neither of pred / pred_scores, non-positive
 *   dimension, unknown dtype, percentile_frac outside [0, 1], has_tolerance outside {0, 1}, negative tol_d2, struct_size below this
 *   version's; UAPS_ERANGE H or W above UAPS_SURFACE_MAX_EXTENT, C outside [1, UAPS_MAX_CLASSES], a tensor or the workspace of 2 GiB
 *   or more (by dimensions); UAPS_EWORKSPACE.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_SURFACE_MAX_EXTENT 4096
#define UAPS_SURFACE_COLUMNS 12
#define UAPS_EDT_NO_FEATURE 1073741824           /* 2^30 */
#define UAPS_LABEL_U8 1
#define UAPS_LABEL_I32 4
#define UAPS_LABEL_I64 8

typedef struct uaps_edt_call {
    uint32_t struct_size;
    int32_t B, H, W;
    int32_t mask_dtype;                          /* UAPS_LABEL_* */
    const void* mask;                            /* [B][H][W] */
    int32_t* out;                                /* [B][H][W] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_edt_call;
int uaps_edt_workspace_bytes(int B, int H, int W, size_t* bytes);
int uaps_edt_sq(const uaps_edt_call* call);

typedef struct uaps_surface_call {
    uint32_t struct_size;
    int32_t B, C, H, W;
    int32_t pred_dtype, target_dtype;            /* UAPS_LABEL_*; pred_dtype is not read with pred_scores */
    const void* pred;                            /* [B][H][W] or NULL */
    const float* pred_scores;                    /* [B][C][H][W] or NULL: exactly one of the two */
    const void* target;                          /* [B][H][W] */
    double percentile_frac;                      /* percentile / 100.0, in [0, 1] */
    int32_t has_tolerance;
    int64_t tol_d2;                              /* floor(tolerance^2) */
    int64_t* table;                              /* [B][C][UAPS_SURFACE_COLUMNS] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_surface_call;
int uaps_surface_workspace_bytes(int B, int C, int H, int W, size_t* bytes);
int uaps_surface_distances(const uaps_surface_call* call);

/* ---------------------------------------------------------------------------------------------
 * Defect matching against ground truth: csrc/match.hip.  Two results of uaps_label_instances over the same B, H, W -- the prediction's
 * (labels, count, table with max_pred rows) and the ground truth's (max_gt rows) -- are matched defect by defect.  Integers throughout.
 *
 *   Pixel rule   a pixel of image b with p = pred_labels, g = target_labels counts iff 1 <= p <= max_pred, 1 <= g <= max_gt and the
 *                class columns of the two table rows are equal (class_agnostic == 1: always); it adds 1 to inter[b, p, g].  Components
 *                numbered above max_instances have no row and take part in nothing.
 *   Match rule   with union = area_p + area_g - inter (areas from the tables), p and g are matched iff
 *                (double) inter > iou_threshold * (double) union -- strict, the panoptic-quality rule; 0.5 <= iou_threshold < 1, where
 *                a component has at most one match (2 inter > union >= area, so more than half of it lies in the partner).
 *     pred_out   int64 [B, max_pred, 4]: partner (the target number with the largest intersection, the lowest on ties, 0: none), inter
 *                (with that partner), covered (the sum of inter[b, p, :]), matched (0 / 1); rows from min(count, max_pred) on are zero
 *     target_out int64 [B, max_gt, 4]: the same from the ground truth's side
 *     counts     int64 [B, num_classes, 3]: tp, n_pred, n_gt per image and class, over the in-table components with a class in
 *                [0, num_classes); tp is attributed to the ground-truth component's class
 *   Launches: zero (the min(count_p, max_pred) x min(count_g, max_gt) corner of every image's pair matrix, from the device-side
 *   counts, and `counts`), the pair count (both label tensors streamed once, four pixels a lane with 16-byte loads where H * W % 4 == 0
 *   and the tensors are 16-byte aligned; one integer atomicAdd per run of equal (p, g) inside a wave, whole waves of one pair carried on in
 *   registers and combined per workgroup in LDS), one reduction per side.  Integer atomics only, no workgroup waits for another: two
 *   runs give the same bits.  The call does not synchronise.
 *   workspace: uaps_match_workspace_bytes(B, max_pred, max_gt) bytes (the dense pair matrix int32 [B, max_pred, max_gt]), 256-byte
 *   aligned, the call's alone until it has run.
 * The struct is size-versioned (fields are only ever appended; a larger struct_size is accepted and what it appends is not read).
 * Errors (nothing launched): UAPS_EINVAL null struct or pointer, non-positive dimension or max_pred / max_gt, struct_size below this
 *   version's, class_agnostic outside {0, 1}, a workspace that is too small or not 256-byte aligned; UAPS_ERANGE num_classes outside
 *   [1, UAPS_MATCH_MAX_CLASSES], H * W >= 2^31, iou_threshold outside [0.5, 1) (NaN included), a pair matrix of
 *   B * max_pred * max_gt * 4 bytes at or beyond 2 GiB.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_MATCH_MAX_CLASSES 64
#define UAPS_MATCH_COLUMNS 4

typedef struct uaps_match_call {
    uint32_t struct_size;
    int32_t B, H, W;
    int32_t num_classes;
    int32_t class_agnostic;                      /* 1: the class test is skipped */
    double iou_threshold;                        /* in [0.5, 1) */
    const int32_t* pred_labels;                  /* [B][H][W] */
    const int32_t* target_labels;                /* [B][H][W] */
    const int32_t* pred_count;                   /* [B] */
    const int32_t* target_count;                 /* [B] */
    const int64_t* pred_table;                   /* [B][max_pred][9] */
    const int64_t* target_table;                 /* [B][max_gt][9] */
    int32_t max_pred, max_gt;
    int64_t* pred_out;                           /* [B][max_pred][4] */
    int64_t* target_out;                         /* [B][max_gt][4] */
    int64_t* counts;                             /* [B][num_classes][3] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_match_call;
int uaps_match_workspace_bytes(int B, int max_pred, int max_gt, size_t* bytes);
int uaps_match_instances(const uaps_match_call* call);

/* ---------------------------------------------------------------------------------------------
 * Defect detection matching over an IoU sweep: csrc/detect.hip.  The COCO assignment step on the pair matrix of uaps_match_instances
 * (same pixel rule, csrc/pair_count.hpp): per image, class and threshold the detections are visited in score order and each takes the
 * not-yet-taken ground-truth defect of largest IoU among those that pass.  Integers throughout (the score key aside), no float compare
 * of IoUs anywhere.
 *
 *   Thresholds   T of them (1 <= T <= UAPS_DETECT_MAX_THRESHOLDS), integers per mille, strictly ascending, each in [100, 1000].
 *   IoU test     1000 * inter >= t1000 * (area_p + area_g - inter), in 64-bit integers; two IoUs are compared by cross-multiplication.
 *   Score key    scores == NULL: (double) sum0 / (double) area of the prediction's table row (one correctly rounded division; the
 *                2^-24 scale of the fixed-point sum is left to whoever shows the score); else scores[b][p].  -0 counts as +0.  A NaN
 *                orders after every number and is written as -inf; rows without a defect hold -inf.
 *   Groups       a defect takes part iff it has a table row and its class lies in [0, num_classes); with class_agnostic == 1 every
 *                defect with a row takes part as class 0.  Within an (image, class) detections are ordered by key descending, the lower
 *                number first on ties; with max_dets = n > 0 only the first n of each (image, class) take part (0: all of them).
 *   Greedy rule  per image, class and threshold, in that order: a detection takes the free ground-truth defect of largest IoU among
 *                those passing the test (the lowest number on ties); a ground-truth defect is taken at most once per threshold.
 *     score      double [B, max_pred]
 *     rank       int64 [B, max_pred]: position within the (image, class), -1 for rows that take no part
 *     pred_match int64 [B, max_pred, T]: the ground-truth number taken, 0: none;  pred_inter: int64 [B, max_pred, T], its intersection
 *     target_match int64 [B, max_gt, T]: the detection number, 0: none
 *     counts     int64 [B, num_classes, T + 2]: tp per threshold, n_pred taking part, n_gt
 *   Launches: the two of the pair count; candidates (one wave per (b, p): the at most UAPS_DETECT_MAX_CANDIDATES = 10 ground-truth
 *   defects that pass the lowest threshold -- inter >= t_min union >= t_min area_p and ground-truth defects are disjoint -- ordered by
 *   (IoU descending, number ascending), and the score key); order (one workgroup per image: rank by counting inside the class, the
 *   class-major sequence, n_pred and n_gt); sweep (one wave per image, lane = threshold, detections in sequence; taken-masks in LDS).
 *   Integer atomics only in the pair count, no workgroup waits for another: two runs give the same bits.  The call does not synchronise.
 *   workspace: uaps_detect_workspace_bytes(B, max_pred, max_gt, T) bytes, 256-byte aligned, the call's alone until it has run.
 * The struct is size-versioned (fields are only ever appended; a larger struct_size is accepted and what it appends is not read).
 * Errors (nothing launched): UAPS_EINVAL null struct or pointer (scores may be null), non-positive dimension or max_pred / max_gt,
 *   struct_size below this version's, class_agnostic outside {0, 1}, negative max_dets, a workspace that is too small or not 256-byte
 *   aligned; UAPS_ERANGE T outside [1, UAPS_DETECT_MAX_THRESHOLDS], a threshold outside [100, 1000] or not above the one before it,
 *   num_classes outside [1, UAPS_MATCH_MAX_CLASSES], max_pred or max_gt above UAPS_DETECT_MAX_ROWS, H * W >= 2^31, a pair matrix of
 *   B * max_pred * max_gt * 4 bytes at or beyond 2 GiB.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_DETECT_MAX_THRESHOLDS 32
#define UAPS_DETECT_MAX_CANDIDATES 10
#define UAPS_DETECT_MAX_ROWS 4096

typedef struct uaps_detect_call {
    uint32_t struct_size;
    int32_t B, H, W;
    int32_t num_classes;
    int32_t class_agnostic;                      /* 1: the class test is skipped and every defect is of class 0 */
    int32_t T;
    int32_t max_dets;                            /* 0: no limit */
    int32_t t1000[UAPS_DETECT_MAX_THRESHOLDS];   /* the first T are read */
    const int32_t* pred_labels;                  /* [B][H][W] */
    const int32_t* target_labels;                /* [B][H][W] */
    const int32_t* pred_count;                   /* [B] */
    const int32_t* target_count;                 /* [B] */
    const int64_t* pred_table;                   /* [B][max_pred][9] */
    const int64_t* target_table;                 /* [B][max_gt][9] */
    int32_t max_pred, max_gt;
    const double* scores;                        /* [B][max_pred], or null: sum0 / area */
    double* score;                               /* [B][max_pred] */
    int64_t* rank;                               /* [B][max_pred] */
    int64_t* pred_match;                         /* [B][max_pred][T] */
    int64_t* pred_inter;                         /* [B][max_pred][T] */
    int64_t* target_match;                       /* [B][max_gt][T] */
    int64_t* counts;                             /* [B][num_classes][T + 2] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_detect_call;
int uaps_detect_workspace_bytes(int B, int max_pred, int max_gt, int T, size_t* bytes);
int uaps_detect_match(const uaps_detect_call* call);

/* ---------------------------------------------------------------------------------------------
 * Threshold-sweep histograms: csrc/curves.hip.  Per image and row the histogram of quantised scores split by a binary event -- the one
 * primitive AUROC, average precision, AUPRO, ECE and AURC are formed from (uaps_amd/curves.py does that on the host, in float64).
 * Integers throughout, pro_sum aside (float64, summed in a fixed order): exact, and the same bits from run to run.
 *
 *   Bin rule   inv = (float) bins / ((float) hi - (float) lo), formed once on the host in fp32;
 *              bin(s) = clamp(floor((s - lo) * inv), 0, bins - 1): subtraction and product rounded separately in fp32 (no fma), the clamp
 *              in float before the conversion.  +inf and everything >= hi land in the last bin, -inf and everything < lo in bin 0; a NaN
 *              enters no bin and is counted in `nan`.  2 <= bins <= UAPS_CURVES_MAX_BINS.
 *   Rows       uaps_score_curves forms R = n_classes + top_row rows per image from one read of scores fp32 [B, C, H, W]:
 *              class row k: score = S[b, classes[k], y, x], event = (target == classes[k]);
 *              top row (C >= 2): score = max_c S[b, c], event = (arg-max_c == target), the lowest index among equal values, taken on
 *                the logits with from_logits; its score is NaN where any of the pixel's C scores is.
 *              A pixel whose target lies outside [0, C) enters no row and no counter.  from_logits == 1: the softmax over the pixel's C
 *              values is formed in registers first.  C == 1 is the sigmoid head: the plane is the score p of class 1
 *              (1 / (1 + expf(-z)) with from_logits), classes is {1}, event = (target == 1), targets outside {0, 1} are ignored; its top
 *              row is score = max(p, 1 - p), event = ((p > 0.5) == target), z > 0 with from_logits.
 *   Plane      uaps_plane_curves: score fp32 [B, H, W] with its own lo / hi, pred and target label maps; one row, event = (pred == target);
 *              pixels with target < 0 are ignored.
 *   Outputs    (the call zeroes them itself) hist int64 [B, R, 2, bins], index 0 = event false, 1 = true; qsum int64 [B, R, 2, bins] or
 *              NULL: the sum over the cell's pixels of q(s) = (int64) rintf(clamp(s, -65536, 65536) * 2^24), the fixed point of
 *              uaps_label_instances; nan int64 [B, R].
 *   Regions    optional, all of region_labels / region_count / region_table (a uaps_label_instances result of the ground truth with
 *              max_regions rows), pro_sum, n_regions and the workspace, or none.  A pixel with region label g in [1, max_regions] whose
 *              region class c = table[b, g - 1, 0] lies in [0, C) (C == 1: equals 1) adds one to region_hist[b, g - 1, bin(S[b, c, y, x])]
 *              (int32 [B, max_regions, bins] in the workspace; only the rows below min(count[b], max_regions) are zeroed and used, the
 *              bound is read on the device).  Then pro_sum float64 [B, n_classes, bins]: pro_sum[b, k, i] = the sum over the regions r of
 *              image b whose class is classes[k], in ascending r, of (double) suffix_r(i) / (double) area_r, suffix_r(i) = sum over
 *              j >= i of region_hist[b, r, j], area_r = table[b, r, 1]; n_regions int64 [B, n_classes] their number.  A row whose
 *              area is not positive is no region: it is not counted and adds nothing.
 *   Launches: zero; one pass over the scores (four pixels a lane with 16-byte loads where H * W % 4 == 0 and the tensors are 16-byte
 *   aligned, rows privatised in at most 64 KB of LDS as 32-bit counters, lanes of a wave with one key counted by ballot, non-zero words
 *   flushed with 64-bit integer atomics; rows that do not fit are processed in groups along the grid's second dimension); with regions
 *   the reduction.  Integer atomics only, nothing waits inside a launch; the call does not synchronise.
 *   workspace: uaps_curves_workspace_bytes(B, max_regions, bins) bytes (0 without regions), 256-byte aligned, the call's alone until it
 *   has run.
 * Both structs are size-versioned (fields are only ever appended; a larger struct_size is accepted and what it appends is not read).
 * Errors (nothing launched): UAPS_EINVAL null struct or a pointer the call uses, non-positive dimension, struct_size below this
 *   version's, unknown dtype, from_logits or top_row outside {0, 1}, from_logits in plane mode, n_classes + top_row == 0 or n_classes
 *   outside [0, UAPS_MAX_CLASSES], a class outside [0, C) (C == 1: other than 1), lo >= hi or a non-finite bound (or a range so narrow
 *   that inv is not finite), regions without all of their operands, a workspace that is too small or not 256-byte aligned;
 *   UAPS_ERANGE C outside [1, UAPS_MAX_CLASSES], bins outside [2, UAPS_CURVES_MAX_BINS], H * W >= 2^31, any tensor or the workspace
 *   at or beyond 2 GiB (by dimensions).
 * ------------------------------------------------------------------------------------------- */
#define UAPS_CURVES_MAX_BINS 4096

typedef struct uaps_curves_call {
    uint32_t struct_size;
    int32_t B, C, H, W;
    int32_t bins;
    int32_t from_logits, top_row;
    int32_t n_classes;
    int32_t classes[UAPS_MAX_CLASSES];
    int32_t target_dtype;                        /* UAPS_LABEL_* */
    float lo, hi;
    const float* scores;                         /* [B][C][H][W] */
    const void* target;                          /* [B][H][W] */
    const int32_t* region_labels;                /* [B][H][W] or NULL */
    const int32_t* region_count;                 /* [B] */
    const int64_t* region_table;                 /* [B][max_regions][9] */
    int32_t max_regions;
    int64_t* hist;                               /* [B][R][2][bins] */
    int64_t* qsum;                               /* [B][R][2][bins] or NULL */
    int64_t* nan;                                /* [B][R] */
    double* pro_sum;                             /* [B][n_classes][bins], with regions */
    int64_t* n_regions;                          /* [B][n_classes], with regions */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_curves_call;
int uaps_curves_workspace_bytes(int B, int max_regions, int bins, size_t* bytes);
int uaps_score_curves(const uaps_curves_call* call);

typedef struct uaps_plane_curves_call {
    uint32_t struct_size;
    int32_t B, H, W;
    int32_t bins;
    int32_t from_logits;                         /* must be 0 */
    int32_t pred_dtype, target_dtype;            /* UAPS_LABEL_* */
    float lo, hi;
    const float* score;                          /* [B][H][W] */
    const void* pred;                            /* [B][H][W] */
    const void* target;                          /* [B][H][W] */
    int64_t* hist;                               /* [B][1][2][bins] */
    int64_t* qsum;                               /* [B][1][2][bins] or NULL */
    int64_t* nan;                                /* [B][1] */
    uaps_stream_t stream;
} uaps_plane_curves_call;
int uaps_plane_curves(const uaps_plane_curves_call* call);

/* ---------------------------------------------------------------------------------------------
 * Defect convex hulls: csrc/hull.hip.
 *
 * uaps_hull_descriptors: the convex hull of every component of the `labels` of uaps_label_instances and what its strict vertices
 *   give: the area, the farthest pair (maximum Feret diameter), the minimum caliper width and the minimum-area rectangle.
 *   labels int32 [B, H, W]: 0 = no component, k >= 1 = component k of that image.
 *   Geometry.  A pixel (y, x) is the closed unit square [x, x + 1] x [y, y + 1]; the hull of component k is the convex hull of the
 *   squares of ALL pixels labelled k, connected or not, so its vertices lie on the corner lattice 0..W x 0..H.  Only strict
 *   vertices count.  Order: v_0 is the smallest vertex (y, then x), v_1 the other end of the horizontal top edge, and so on
 *   (clockwise on the screen).  Edge i runs from v_i to v_{i+1} (cyclic) with the vector e = (ex, ey); for a point p
 *     c(p) = ex (py - vy) - ey (px - vx)  (>= 0 on the hull),   d(p) = ex (px - vx) + ey (py - vy).
 *     table int64 [B, max_instances, 17]   row k - 1 of image b, 1 <= k <= max_instances:
 *       0      nv        the number of strict vertices (>= 4)
 *       1      area2     twice the hull's area: the shoelace sum
 *       2..6   fmax_sq, f_y0, f_x0, f_y1, f_x1   the largest squared distance between two vertices and the pair that attains
 *                        it, (y0, x0) < (y1, x1) lexicographically; among tied pairs the smallest (y0, x0, y1, x1)
 *       7..9   w_ey, w_ex, w_c   the edge that minimises C^2 / |e|^2, C the largest c(p) over the vertices: its vector and C.
 *                        The minimum caliper width is w_c / |e|
 *       10..16 r_y, r_x, r_ey, r_ex, r_dmin, r_dmax, r_c   the edge that minimises (dmax - dmin) C / |e|^2, dmin and dmax the
 *                        extremes of d(p) over the vertices: its start vertex, its vector, dmin <= 0, dmax and C.  The
 *                        minimum-area rectangle is flush with that edge; its sides are (dmax - dmin) / |e| and C / |e|
 *     Both minimisations compare the fractions exactly (cross-multiplied in 128-bit integers); ties go to the edge with the
 *     lowest index.  A label <= 0 or above max_instances has no row.  Rows without a pixel are zero; every row is written once,
 *     whatever table and workspace held before.  All columns are exact integers; no float is used.
 *   Three launches: the workspace is zeroed; one pass over the labels raises, per run of equal labels along a row, the column
 *   extents of that (image, component, row) and the row range of the component with integer atomicMax (the minima are stored
 *   inverted); one workgroup per (image, component) builds the two chains of lattice-line extremes in LDS (8 (H + 1) bytes),
 *   reduces them to the strict vertices and evaluates the columns.  The same bits from run to run.  The call does not synchronise.
 *   workspace: uaps_hull_workspace_bytes(B, H, W, max_instances) = B * max_instances * (H + 1) * 8 bytes (rounded up to 256),
 *   256-byte aligned, the call's alone until it has run; it need not be zeroed.
 * Errors (nothing launched): UAPS_EINVAL null struct, labels, table or workspace (the query: a NULL result pointer), table ==
 *   labels, non-positive dimension, max_instances < 1, struct_size below this version's; UAPS_ERANGE H or W above
 *   UAPS_HULL_MAX_EXTENT, B * H * W * 8 >= 2 GiB, a table or a workspace of 2 GiB or more (by dimensions); UAPS_EWORKSPACE a
 *   workspace smaller than that or not 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_HULL_COLUMNS 17
#define UAPS_HULL_MAX_EXTENT 4096
typedef struct uaps_hull_call {
    uint32_t struct_size;
    int32_t B, H, W, max_instances;
    const int32_t* labels;                       /* [B][H][W] */
    int64_t* table;                              /* [B][max_instances][17], written whole */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_hull_call;
int uaps_hull_workspace_bytes(int B, int H, int W, int max_instances, size_t* bytes);
int uaps_hull_descriptors(const uaps_hull_call* call);

/* ---------------------------------------------------------------------------------------------
 * Defect contours: csrc/contours.hip.
 *
 * uaps_contours_trace / uaps_contours_write: the boundary of every component of the `labels` of uaps_label_instances as closed
 *   rings of corner-lattice points, outer rings and hole rings, exact integers.
 *   labels int32 [B, H, W]: 0 = no component, k >= 1 = component k of that image.
 *   Geometry.  A pixel (y, x) is the closed unit square [x, x + 1] x [y, y + 1]; ring points lie on the corner lattice 0..H x 0..W
 *   and are stored (y, x).  For a label k, 1 <= k <= max_instances, every unit side between a pixel of k and anything else (another
 *   label, 0, a label outside [1, max_instances], the frame) is a directed edge with k on its right; directions E, S, W, N = 0..3:
 *     top side of (y, x): from (y, x) heading E;          right side: from (y, x + 1) heading S;
 *     bottom side:        from (y + 1, x + 1) heading W;  left side:  from (y + 1, x) heading N.
 *   Outer rings run clockwise on the screen (as the hull does), hole rings counter-clockwise.  The next edge leaves the end vertex
 *   of this one; it is unique but at a saddle vertex (k on exactly the two diagonal pixels of the 2 x 2 window), where
 *   connectivity 8 turns left (d + 3 mod 4: the diagonal pixels stay on one ring) and connectivity 4 right (d + 1).  A ring is one
 *   cycle of that map.  It starts at its smallest vertex (y, then x), which it visits once: outer rings leave it heading E, hole
 *   rings heading S.  Rings are ordered by (image, start y, start x, direction of the start edge) -- a raster order, not grouped
 *   by label.
 *     points       int32 [N, 2]   the start vertices (y, x) of the edges whose direction differs from their predecessor's, ring after
 *                                 ring, from the ring's start; the first point is not repeated.  Even and >= 4 a ring; a saddle
 *                                 vertex can occur twice
 *     ring_offsets int32 [L + 1]  ring r owns points[ring_offsets[r] .. ring_offsets[r + 1])
 *     rings        int64 [L, 7]   image, label, start y, start x, points, length (unit edges), area2 (the shoelace sum
 *                                 x y' - x' y over the edges: twice the enclosed area, > 0 for outer rings, < 0 for holes)
 *     summary      int64 [B, max_instances, 4]   per label the sums over its rings: rings, points, perimeter (= sum of length),
 *                                 area2 (= twice the label's pixel count); zero rows for labels without a pixel
 *     totals       int64 [4]      L, N, the doubling rounds that ran, the number of directed edges
 *   uaps_contours_trace fills the workspace, `summary` and `totals` (on the device); it does not synchronise.  The caller reads
 *   L and N from `totals`, provides points / ring_offsets / rings of at least that capacity and passes both the totals it read
 *   (n_rings, n_points) and the capacities to uaps_contours_write, which fills them from the SAME, untouched workspace with one
 *   launch.  With L = 0 there is nothing to write (n_rings < 1 is refused).  A workspace whose totals are not the ones passed
 *   makes the launch store nothing.  Every output word is written once, whatever outputs and workspace held before; the same
 *   bits from run to run; no float is used.
 *   Passes: a scan of per-vertex edge counts compacts the edges in key order (image, start vertex, direction); every edge names
 *   its successor from the 2 x 2 window at its end vertex; pointer doubling along the predecessors, one launch a round (at most
 *   ceil(log2(4 H W)); a launch returns at once after a round that changed nothing, without a host read), gives every edge its
 *   ring's smallest edge and its rank from it; two more scans give ring indices, point slots and the shoelace sums.
 *   workspace: uaps_contours_workspace_bytes(B, H, W, max_instances): about 192 bytes a pixel and 4 a lattice vertex, 256-byte
 *   aligned, the pair of calls' alone from trace until write has run; it need not be zeroed.
 * Errors (nothing launched, outputs untouched): UAPS_EINVAL null struct, labels or workspace, trace: null summary or totals or two
 *   of labels / summary / totals equal, write: null points, ring_offsets or rings, n_rings < 1, n_points < 4, a total of 2^31 or
 *   more, ring_capacity < n_rings or point_capacity < n_points; non-positive dimension, max_instances < 1, connectivity not 4 or
 *   8, struct_size below this version's (the query: a NULL result pointer); UAPS_ERANGE H or W above UAPS_CONTOUR_MAX_EXTENT,
 *   B * H * W * 32 >= 2 GiB (every workspace array stays below 2 GiB), a summary of 2 GiB or more; UAPS_EWORKSPACE a workspace
 *   smaller than the query's answer or not 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_CONTOUR_COLUMNS 4
#define UAPS_CONTOUR_RING_COLUMNS 7
#define UAPS_CONTOUR_MAX_EXTENT 4096
typedef struct uaps_contour_call {
    uint32_t struct_size;
    int32_t B, H, W, max_instances, connectivity;
    const int32_t* labels;                       /* [B][H][W] */
    int64_t* summary;                            /* trace: [B][max_instances][4], written whole */
    int64_t* totals;                             /* trace: [4] on the device */
    int64_t n_rings, n_points;                   /* write: L and N as read from totals */
    int64_t ring_capacity, point_capacity;       /* write: rows of rings (ring_offsets has one more) and of points */
    int32_t* points;                             /* write: [point_capacity][2] */
    int32_t* ring_offsets;                       /* write: [ring_capacity + 1] */
    int64_t* rings;                              /* write: [ring_capacity][7] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_contour_call;
int uaps_contours_workspace_bytes(int B, int H, int W, int max_instances, size_t* bytes);
int uaps_contours_trace(const uaps_contour_call* call);
int uaps_contours_write(const uaps_contour_call* call);

/* ---------------------------------------------------------------------------------------------
 * Contour simplification: csrc/simplify.hip.
 *
 * uaps_contours_simplify_mark / uaps_contours_simplify_write: exact Ramer-Douglas-Peucker on the rings of uaps_contours_write;
 *   integers only, the same bits from run to run and from every kernel form.
 *   Inputs: points int32 [n_points, 2] (y, x), coordinates in 0 .. UAPS_CONTOUR_MAX_EXTENT; ring_offsets int32 [n_rings + 1];
 *   rings int64 [n_rings, 7]; summary_in int64 [B, max_instances, 4] -- the outputs of uaps_contours_trace / _write.
 *   A ring has n >= 4 points p_0 .. p_{n-1}; index n means p_0 again.  e16 is the tolerance in sixteenths of a pixel, 0 .. 1024.
 *   Deviation of P from the SEGMENT A -> B as a fraction num / den of squared pixels, d = B - A, L2 = |d|^2, t = (P - A) . d:
 *     L2 == 0: num = |P - A|^2, den = 1;   t <= 0: num = |P - A|^2 L2, den = L2;   t >= L2: num = |P - B|^2 L2, den = L2;
 *     otherwise num = cross(d, P - A)^2, den = L2.            (num <= 2^50: every comparison stays inside int64)
 *   P exceeds the tolerance where 256 num > e16^2 den (strict).
 *   Split rule, for an interval (i, j) of kept indices with j > i + 1: the interior index k with the largest num (den is common),
 *   the lowest k among the equal; if it exceeds the tolerance k is kept and the rule goes on in (i, k) and (k, j), otherwise
 *   nothing inside is kept.  A ring keeps 0 and b, the index with the largest |p_i - p_0|^2 (the lowest among the equal), and runs
 *   the rule on (0, b) and (b, n).  If neither splits, the index with the largest num over both (they share the segment; the
 *   lowest among the equal) is kept all the same and the rule goes on in its two halves: a ring never falls below a triangle, and
 *   every dropped point stays within the tolerance of the segment between the kept points that bracket it.
 *   NOT promised: a simplified ring may touch or cross itself or another ring, and the sign of its own area can change.
 *     points_out       int32 [N', 2]           the kept points in source order, ring after ring, p_0 first
 *     ring_offsets_out int32 [n_rings + 1]
 *     rings_out        int64 [n_rings, 7]      the source rows with column `points` = the kept count; length and area2 stay the
 *                                              traced ring's
 *     ring_stats       int64 [n_rings, 2]      points of the source ring, the shoelace sum of the simplified ring
 *     summary_out      int64 [B, max_instances, 4]   summary_in with kept - n of every ring added to column `points`
 *     totals           int64 [4]               n_rings, N', the rings that took the LDS form, the rings that took the global form
 *   uaps_contours_simplify_mark copies the summary, runs the split rule, counts and scans the kept points and fills `totals` (on
 *   the device); it does not synchronise.  The caller reads N' from `totals`, provides the outputs and passes n_points_out = N' and
 *   the capacities to uaps_contours_simplify_write, which fills them from the SAME, untouched workspace with one launch.  A
 *   workspace whose total is not the one passed makes the launch store nothing.
 *   Forms, by a ring's point count n: n <= wave_max one ring a wave (a point a lane); n <= lds_max one ring a workgroup with its
 *   state in LDS; any n one ring a workgroup with its state in the workspace.  wave_max / lds_max: 0 = the default
 *   (UAPS_SIMPLIFY_WAVE_MAX, UAPS_SIMPLIFY_LDS_MAX), UAPS_SIMPLIFY_OFF = no ring takes the form; they change the time, never a bit.
 *   workspace: uaps_contours_simplify_workspace_bytes(n_points, n_rings): about 28 bytes a point and 24 a ring, 256-byte aligned,
 *   the pair of calls' alone from mark until write has run; it need not be zeroed.
 * Errors (nothing launched, outputs untouched): UAPS_EINVAL null struct, points, ring_offsets, rings or workspace, B or
 *   max_instances < 1, n_points or n_rings < 1, e16 outside 0 .. UAPS_SIMPLIFY_MAX_E16, wave_max / lds_max above the form's capacity
 *   or below UAPS_SIMPLIFY_OFF, struct_size below this version's, mark: null summary_in, summary_out or totals or two of them equal,
 *   write: a null output, n_points_out < 1 or above n_points, ring_capacity < n_rings or point_capacity < n_points_out;
 *   UAPS_ERANGE n_points of 2^30 or more, more rings than points, a summary of 2 GiB or more; UAPS_EWORKSPACE a workspace smaller
 *   than the query's answer or not 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_SIMPLIFY_WAVE_MAX 64
#define UAPS_SIMPLIFY_LDS_MAX 2048
#define UAPS_SIMPLIFY_MAX_E16 1024
#define UAPS_SIMPLIFY_OFF (-1)
typedef struct uaps_simplify_call {
    uint32_t struct_size;
    int32_t B, max_instances;                    /* the summary's rows */
    int32_t e16;
    int32_t wave_max, lds_max;
    int64_t n_points, n_rings;
    const int32_t* points;                       /* [n_points][2] */
    const int32_t* ring_offsets;                 /* [n_rings + 1] */
    const int64_t* rings;                        /* [n_rings][7] */
    const int64_t* summary_in;                   /* mark: [B][max_instances][4] */
    int64_t* summary_out;                        /* mark: [B][max_instances][4], written whole */
    int64_t* totals;                             /* mark: [4] on the device */
    int64_t n_points_out;                        /* write: N' as read from totals */
    int64_t ring_capacity, point_capacity;       /* write: rows of rings_out and ring_stats (ring_offsets_out has one more), of points_out */
    int32_t* points_out;                         /* write: [point_capacity][2] */
    int32_t* ring_offsets_out;                   /* write: [ring_capacity + 1] */
    int64_t* rings_out;                          /* write: [ring_capacity][7] */
    int64_t* ring_stats;                         /* write: [ring_capacity][2] */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_simplify_call;
int uaps_contours_simplify_workspace_bytes(int64_t n_points, int64_t n_rings, size_t* bytes);
int uaps_contours_simplify_mark(const uaps_simplify_call* call);
int uaps_contours_simplify_write(const uaps_simplify_call* call);

/* ---------------------------------------------------------------------------------------------
 * Polygon rasterisation: csrc/raster.hip.
 *
 * uaps_raster_plan / uaps_raster_fill: the exact even-odd fill of polygon rings into a label map -- the inverse of
 *   uaps_contours_trace / _write; integers only, the same bits from run to run and from both edge forms.
 *   Inputs: points int32 [n_points, 2] (y, x) in units of 2^-frac_bits pixel, 0 <= y, x <= UAPS_RASTER_MAX_EXTENT << frac_bits
 *   (values outside are clamped into that range); ring_offsets int32 [n_rings + 1]; rings int64 [n_rings, ring_stride] with the
 *   image in column 0 and the label in column 1 (ring_stride 7: the rings of uaps_contours_write and uaps_contours_simplify_write).
 *   A ring of n points has n edges, the last one closes it; rings of fewer than 3 points, of an image outside [0, B) or of a label
 *   outside [1, max_instances] contribute nothing.  Rings may reach outside the H x W frame.
 *   Pixel (r, c) is sampled at its centre (r + 1/2, c + 1/2).  In doubled units with s = 2^frac_bits a row's centre is
 *   Yc = (2 r + 1) s; an edge A -> B crosses row r iff min(2 ya, 2 yb) <= Yc < max(2 ya, 2 yb) (half-open: a vertex on a centre
 *   row counts once, horizontal edges never cross); with (Y0, X0) the doubled endpoint of smaller Y, dy > 0 and dx the doubled
 *   differences to the other one and num = X0 dy + (Yc - Y0) dx, the first column at or right of the crossing is
 *   c0 = ceil((num - s dy) / (2 s dy)) clamped to [0, W] (a centre exactly on an edge counts as right of it; c0 = W toggles nothing).
 *   Even-odd per label: pixel (r, c) belongs to label k iff the number of crossings of k's edges in row r with c0 <= c is odd.
 *     labels   int64 [B, H, W]                the lowest label that owns the pixel, `background` where none does
 *     mask     int64 [B, H, W]                with classes (int64 [B, max_instances]): classes[b][label - 1], 0 where no label owns it
 *     stats    int64 [B, max_instances, 2]    area (the pixels the label owns, whatever other labels own them too), inter (those of
 *                                             them where reference == label; 0 without a reference)
 *     overlap  int64 [B]                      the pixels owned by more than one label
 *     totals   int64 [4]                      the 64-bit words of all bit planes, the labels with a word, their box rows, 0
 *   uaps_raster_plan finds the box of every label's ring points clipped to the frame -- rows x 64-bit words, one bit a pixel --
 *   scans the words into offsets and fills `totals` (on the device); it does not synchronise.  The caller reads totals[0], provides
 *   `planes` of that many words and passes n_words to uaps_raster_fill, which fills the outputs from the SAME, untouched workspace:
 *   planes cleared, every row an edge crosses toggles bit c0 of the label's box row (64-bit atomic XOR), a prefix XOR along every
 *   box row, set pixels to a paint plane by atomicMin, the paint plane to labels.  ring_offsets is not validated: points that no
 *   ring [ring_offsets[r], ring_offsets[r + 1]) inside [0, n_points] holds are left out, silently.  With totals[0] = 0 no pixel is owned and there
 *   is nothing to fill (n_words < 1 is refused).  A workspace whose total is not the one passed makes the launches store nothing.
 *   edge_wave_rows: an edge that crosses more rows than this goes on a list that a second launch deals to whole waves, an edge a
 *   wave; 0 = the default (UAPS_RASTER_WAVE_ROWS),
 *   UAPS_RASTER_ALL_WAVE = every edge; it changes the time, never a bit.
 *   workspace: uaps_raster_workspace_bytes(n_points, n_rings, B, H, W, max_instances): 8 bytes a point, 4 a pixel and 24 an
 *   (image, label) pair, 256-byte aligned, the pair of calls' alone from plan until fill has run; it need not be zeroed.
 * Errors (nothing launched, outputs untouched): UAPS_EINVAL null struct, points, ring_offsets, rings or workspace or two of the three
 *   equal, non-positive dimension, max_instances < 1, n_points or n_rings < 1, frac_bits outside 0 .. UAPS_RASTER_MAX_FRAC_BITS,
 *   ring_stride outside 2 .. 64, edge_wave_rows outside UAPS_RASTER_ALL_WAVE .. UAPS_RASTER_MAX_EXTENT, struct_size below this
 *   version's, plan: null totals or totals equal to an input, fill: null planes, labels, stats or overlap, classes without mask or
 *   mask without classes, an output equal to an input or to another output, n_words < 1 (the query: a NULL result pointer);
 *   UAPS_ERANGE H or W above UAPS_RASTER_MAX_EXTENT, n_points or n_rings of 2^30 or more, labels (B * H * W * 8) or the sums
 *   (B * max_instances * 16) of 2 GiB or more, fill: planes (n_words * 8) of 2 GiB or more; UAPS_EWORKSPACE a workspace smaller than
 *   the query's answer or not 256-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define UAPS_RASTER_COLUMNS 2
#define UAPS_RASTER_MAX_EXTENT 4096
#define UAPS_RASTER_MAX_FRAC_BITS 4
#define UAPS_RASTER_WAVE_ROWS 64
#define UAPS_RASTER_ALL_WAVE (-1)
typedef struct uaps_raster_call {
    uint32_t struct_size;
    int32_t B, H, W, max_instances;
    int32_t frac_bits, ring_stride, edge_wave_rows;
    int64_t n_points, n_rings;
    const int32_t* points;                       /* [n_points][2] */
    const int32_t* ring_offsets;                 /* [n_rings + 1] */
    const int64_t* rings;                        /* [n_rings][ring_stride] */
    int64_t* totals;                             /* plan: [4] on the device */
    int64_t n_words;                             /* fill: totals[0] as read */
    uint64_t* planes;                            /* fill: [n_words], the caller's; holds nothing of use afterwards */
    const int32_t* reference;                    /* fill: [B][H][W] or NULL */
    const int64_t* classes;                      /* fill: [B][max_instances] or NULL */
    int64_t background;                          /* fill */
    int64_t* labels;                             /* fill: [B][H][W], written whole */
    int64_t* mask;                               /* fill: [B][H][W], written whole; with classes */
    int64_t* stats;                              /* fill: [B][max_instances][2], written whole */
    int64_t* overlap;                            /* fill: [B], written whole */
    void* workspace;
    size_t workspace_bytes;
    uaps_stream_t stream;
} uaps_raster_call;
int uaps_raster_workspace_bytes(int64_t n_points, int64_t n_rings, int B, int H, int W, int max_instances, size_t* bytes);
int uaps_raster_plan(const uaps_raster_call* call);
int uaps_raster_fill(const uaps_raster_call* call);

#ifdef __cplusplus
}
#endif
#endif /* UAPS_HIP_H */
