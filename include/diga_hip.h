/*
 * diga_hip.h -- C ABI of libdiga_hip.so: the MI355X (gfx950) kernels of the DiGA
 * training hot path.
 *
 * The reference (fy-vision/DiGA) has no FFI: every function below replaces a piece of
 * Python/torch code of the reference, cited as file:line under /root/reference with
 *   G5/ = domain_adaptation/GTA5/.
 * The host-side mirror of the reference interface (diga_amd/util/loss.py, util/utils.py,
 * calc_centroids.py, model/model_noaux.py) binds these entry points with ctypes; see
 * INTEGRATION.md for the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name starts with h_;
 *   - tensors are contiguous; image tensors NCHW fp32 unless the name says nhwc;
 *     labels are int64 as the reference's loaders produce them (255 = ignore);
 *   - the caller owns every buffer, including workspaces (size queries below);
 *     kernels never allocate, free or keep pointers past return;
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*);
 *     no entry point synchronises;
 *   - return 0 on success, a negative DIGA_E* code on a bad argument, or the positive
 *     hipError_t of a failed launch; diga_last_error_string() describes the last failure
 *     of the calling thread.  Nothing throws across the ABI.
 */
#ifndef DIGA_HIP_H
#define DIGA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libdiga_hip.so is built with -fvisibility=hidden: the functions declared in this header are its whole dynamic symbol table */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define DIGA_ABI_VERSION 1

#define DIGA_OK 0
#define DIGA_EINVAL (-1)   /* bad shape / null pointer / unsupported size */
#define DIGA_EALIGN (-2)   /* pointer not aligned as required             */
#define DIGA_EWORKSPACE (-3) /* workspace too small                       */

#define DIGA_IGNORE_LABEL 255

int diga_version(void);
const char* diga_last_error_string(void);

/* ------------------------------------------------------------------------------------
 * Losses
 * ---------------------------------------------------------------------------------- */

/* Bytes of workspace the loss entry points need for `n_pixels` = N*H*W pixels. */
size_t diga_loss_workspace_bytes(int64_t n_pixels);

/* cross_entropy2d, G5/util/loss.py:48-62.
 *   loss      = sum over pixels with target != 255 of -log_softmax(logits)[target] / (N*H*W)
 *   grad      = d loss / d logits * grad_scale      (nullable: loss only)
 * logits [N,C,H,W], target [N,H,W] int64, loss_out [1], C <= 32. */
int diga_ce2d_fwd_bwd(const float* logits, const int64_t* target, float* grad, float* loss_out,
                      void* workspace, size_t workspace_bytes,
                      int64_t N, int64_t C, int64_t H, int64_t W, float grad_scale, void* stream);

/* OhemCrossEntropy (hard-pixel CE of the Synthia / semi-supervised trees), G5/util/loss.py:65-122
 * (`_ohem_forward` :91-109): over pixels with target != ignore_label, p_t = softmax(logits)[target];
 * kth = the min(min_kept, n_valid-1)-th smallest p_t (0-based); thr = max(kth, thresh);
 *   loss = mean of -log_softmax(logits)[target] over the valid pixels with p_t < thr   (NaN if there are none)
 *   grad = d loss / d logits * grad_scale                                               (nullable: loss only)
 * logits [N,C,H,W] at label resolution, target [N,H,W] int64, loss_out [1].  The order statistic is found by an
 * exact radix select on the device (no sort, no host sync). */
size_t diga_ohem_ce_workspace_bytes(int64_t N, int64_t H, int64_t W);
int diga_ohem_ce_fwd_bwd(const float* logits, const int64_t* target, float* grad, float* loss_out,
                         void* workspace, size_t workspace_bytes, int64_t N, int64_t C, int64_t H, int64_t W,
                         int64_t ignore_label, float thresh, int64_t min_kept, float grad_scale, void* stream);

/* distillation_loss, G5/util/loss.py:125-143.  teacher/student [2B,C,H,W]; the two halves of
 * the batch are the two views.  loss = mean_{B,H,W} sum_c -q0 log p1 + scale * mean sum_c -q1 log p0
 * with q = softmax(teacher), p = softmax(student); grad (nullable) = d loss / d student * grad_scale. */
int diga_distill_fwd_bwd(const float* teacher, const float* student, float* grad, float* loss_out,
                         void* workspace, size_t workspace_bytes,
                         int64_t B2, int64_t C, int64_t H, int64_t W, float scale, float grad_scale,
                         void* stream);

/* x *= *scale_dev, skipped entirely (no traffic) when *scale_dev == 1.  Used by the autograd
 * wrappers to apply the upstream gradient without a host sync. */
int diga_scale_inplace(float* x, const float* scale_dev, int64_t n, void* stream);

/* Loss block of the training step at the LOW-RES boundary: bilinear(align_corners=True)
 * upsampling of student and teacher logits to label size fused with both losses and their
 * backward (G5/train_DiGA_gta2city_warm_up.py:173-176,267-282,299).
 *   stu_lr, tea_lr [2B,C,h,w]; labels [B,H,W] int64
 *   losses_out[0] = cross_entropy2d(up(stu)[:B], labels); losses_out[1] = distillation_loss(up(tea), up(stu), scale)
 *   grad_stu_lr [2B,C,h,w] = d(lambda_seg*ce + lambda_distil*distil)/d stu_lr
 * Deterministic (no float atomics).  Requires h,w >= 2. */
size_t diga_upsample_loss_workspace_bytes(int64_t B2, int64_t C, int64_t h, int64_t w);
int diga_upsample_ce_distill_fwd_bwd(const float* stu_lr, const float* tea_lr, const int64_t* labels,
                                     float* grad_stu_lr, float* losses_out,
                                     void* workspace, size_t workspace_bytes,
                                     int64_t B, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                                     float lambda_seg, float lambda_distil, float scale, void* stream);

/* Same fusion for one cross_entropy2d term only (self-training: CE of the cross-domain mix,
 * G5/train_DiGA_gta2city_self_training.py:343-351).  logits_lr [N,C,h,w], labels [N,H,W]. */
int diga_upsample_ce_fwd_bwd(const float* logits_lr, const int64_t* labels, float* grad_lr,
                             float* loss_out, void* workspace, size_t workspace_bytes,
                             int64_t N, int64_t C, int64_t h, int64_t w, int64_t H, int64_t W,
                             float lambda_seg, void* stream);

/* nn.Upsample(size, 'bilinear', align_corners=True) forward (used for eval / drop-in callers). */
int diga_upsample_bilinear_ac(const float* x, float* y, int64_t NC, int64_t h, int64_t w,
                              int64_t H, int64_t W, void* stream);

/* ------------------------------------------------------------------------------------
 * EMA teacher and SGD (multi-tensor; tables are device arrays prepared by the caller)
 * ---------------------------------------------------------------------------------- */

/* update_teacher_params, G5/util/utils.py:103-116:  t <- alpha*t + (1-alpha)*s  (bit-exact to the
 * two-multiply-one-add fp32 arithmetic of the reference).  one_minus_alpha is passed explicitly
 * because the reference rounds (1 - alpha) in double before casting. */
int diga_ema_update_flat(float* teacher, const float* student, int64_t n, float alpha,
                         float one_minus_alpha, void* stream);

/* Same over a list of tensors.  Chunk c covers elements [chunk_start[c], +chunk_elems) of tensor
 * chunk_tensor[c]; sizes[i] = numel of tensor i. */
int diga_ema_update_multi(float* const* teacher_ptrs, const float* const* student_ptrs,
                          const int64_t* sizes, const int32_t* chunk_tensor, const int64_t* chunk_start,
                          int64_t n_chunks, int64_t chunk_elems, float alpha, float one_minus_alpha,
                          void* stream);

/* torch.optim.SGD(momentum, weight_decay) as the reference drives it (G5/model/model_noaux.py:48-77,
 * G5/train_DiGA_gta2city_warm_up.py:156,301-305): tensor i occurs mult[i] times in its group, so one
 * step() is mult[i] sequential micro-steps  d = g + wd*p; buf = first_step ? d : momentum*buf + d;
 * p -= lr[i]*buf  fused in registers.  lr[i] is a device array (per tensor; poly-LR is written there
 * by the host each step).  skip_flag (nullable, device int32): when skip_flag[0] != 0 the launch changes nothing -- the
 * "found_inf" of a loss-scaled fp16 backward (the MiT student, diga_mit.h), decided on the device without a host sync. */
int diga_sgd_momentum_multi(float* const* param_ptrs, const float* const* grad_ptrs, float* const* buf_ptrs,
                            const int64_t* sizes, const int32_t* mult, const float* lr,
                            const int32_t* chunk_tensor, const int64_t* chunk_start,
                            int64_t n_chunks, int64_t chunk_elems,
                            float momentum, float weight_decay, int first_step, float grad_scale,
                            const int32_t* skip_flag, void* stream);
/* flag[0] = 1 and flag[1] += 1 when the n floats at x hold an inf or a NaN (flag: two device int32, zeroed by the caller at
 * the start of a step; [1] counts the overflowed steps).  The reference is fp32 throughout and has no such failure mode
 * (torch.cuda.amp.GradScaler is what a mixed-precision port of it would use: same found_inf / skipped-step semantics). */
int diga_nonfinite_flag_f32(const float* x, int64_t n, int32_t* flag, void* stream);

/* ------------------------------------------------------------------------------------
 * ClassMix (G5/train_DiGA_gta2city_warm_up.py:240-259, ..._self_training.py:259-275,306-325)
 * ---------------------------------------------------------------------------------- */

/* hist[b][v] = number of pixels of image b with label v, v in 0..255 (other values are not
 * counted).  hist [B,256] uint32 must be zeroed by the caller (hipMemsetAsync). */
int diga_label_hist256(const int64_t* labels, uint32_t* hist, int64_t B, int64_t HW, void* stream);

/* out[b,c,y,x] = lut[b][label[b,y,x]] ? fg : bg.  lut [B,256] uint8; bg, fg, out [B,CH,H*W].
 * If labels_out != NULL also labels_out = lut ? labels : bg_labels (label paste of the
 * self-training mix).  Labels outside 0..255 select bg. */
int diga_classmix_paste(const float* bg, const float* fg, const int64_t* labels, const uint8_t* lut,
                        float* out, const int64_t* bg_labels, int64_t* labels_out,
                        int64_t B, int64_t CH, int64_t HW, void* stream);

/* ------------------------------------------------------------------------------------
 * Centroid pseudo-labeler (G5/calc_centroids.py:120-176, ..._self_training.py:298-341)
 * ---------------------------------------------------------------------------------- */

/* Class_Features.get_centroid_weight: w[n,k,p] = softmax_k( -|| centroids[k] - feat[n,:,p] ||_2 ).
 * feat [N,D,HW], centroids [K,D], weights [N,K,HW]; K <= 32.  neg_dist (nullable) receives -d. */
int diga_centroid_softmax_weights(const float* feat, const float* centroids, float* weights,
                                  float* neg_dist, int64_t N, int64_t D, int64_t K, int64_t HW,
                                  void* stream);

/* Bilateral consensus: argmax_k of the bilinear(align_corners) upsampling of weights to [H,W],
 * pseudo_out = pseudo_in where it equals that argmax else 255; feat_pseudo (nullable) = argmax. */
int diga_upsample_argmax_consensus(const float* weights, const int64_t* pseudo_in, int64_t* pseudo_out,
                                   int64_t* feat_pseudo, int64_t N, int64_t K, int64_t h, int64_t w,
                                   int64_t H, int64_t W, void* stream);

/* Class_Features.calculate_mean_vector.  ids[n,p] = argmax_k out[n,k,p], kept only where it equals
 * the label (labels given) and < K.  Labels come either already at feature resolution
 * (labels_lr [N,hw] float, as the reference passes them) or at full resolution (labels_full
 * [N,H,W] int64, nearest-downsampled here with src = floor(dst*in/out)); both NULL = no labels.
 * sums [N,K,D] = sum of feat over member pixels, counts [N,K] (int32). */
size_t diga_class_mean_workspace_bytes(int64_t N, int64_t hw);
int diga_class_mean_vectors(const float* feat, const float* out, const float* labels_lr,
                            const int64_t* labels_full, float* sums, int32_t* counts,
                            void* workspace, size_t workspace_bytes,
                            int64_t N, int64_t D, int64_t K, int64_t h, int64_t w, int64_t H, int64_t W,
                            void* stream);

/* update_objective_SingleVector applied sequentially in image-major / class-minor order:
 * for n, for t: skip if counts<min_pixels or sum(v)==0; v = sums/counts;
 *   mode 0 (moving average): c_t = c_t*(1-m) + m*v ; num_t = min(num_t+1, 3000)
 *   mode 1 (mean):           c_t = (c_t*num_t + v)/(num_t+1) ; num_t = min(num_t+1, 3000)
 * centroids [K,D], nums [K] float. */
int diga_centroid_ema_apply(float* centroids, float* nums, const float* sums, const int32_t* counts,
                            int64_t N, int64_t K, int64_t D, int64_t hw, float momentum, int min_pixels,
                            int mode, void* stream);

/* ------------------------------------------------------------------------------------
 * Metrics (G5/util/metrics.py:32-44)
 * ---------------------------------------------------------------------------------- */

/* hist[gt*K+pred] += 1 for pixels with 0 <= gt < K.  hist [K*K] int64, accumulated into. */
int diga_confusion_matrix(const int64_t* gt, const int64_t* pred, int64_t* hist, int64_t n, int64_t K,
                          void* stream);

/* Two-scale evaluation (G5/train_DiGA_gta2city_warm_up.py:346-359, G5/evaluate_val.py:73-93): per label pixel,
 * argmax_k max(up(pred_a)[k], up(pred_b)[k]) with up = bilinear align_corners upsampling to [H,W]; pred_out
 * (nullable) receives it, hist (nullable, [K*K] int64, accumulated) the confusion against gt (nullable). */
int diga_two_scale_confusion(const float* pred_a, int64_t ha, int64_t wa, const float* pred_b, int64_t hb, int64_t wb,
                             const int64_t* gt, int64_t* pred_out, int64_t* hist, int64_t N, int64_t K, int64_t H,
                             int64_t W, void* stream);

/* ------------------------------------------------------------------------------------
 * Convolution on the fp32 matrix cores (nn.Conv2d layers of G5/model/seg_model_noaux.py:57-101,
 * :140-172; cuDNN in the reference).  Activations NHWC fp32 with a leading dimension (`*_ld` floats
 * between pixels, so channel slices of wider tensors can be read/written in place); weights
 * [Cout][R][S][Cin] = the channels_last image of torch's [Cout,Cin,R,S].
 * ---------------------------------------------------------------------------------- */

/* out[n,ho,wo,k] = bias[k] + sum_{r,s,c} in[n, ho*stride_y + off_y0 + r*off_dy, wo*stride_x + off_x0 + s*off_dx, c]
 *                                        * wgt[k][r][s][c]          (taps outside the image read zero)
 * Forward conv: off_*0 = -padding, off_d* = dilation.  Backward-data of a stride-1 conv: in = dy,
 * wgt = the [Cin][R][S][Cout] transpose (diga_weight_transpose), off_*0 = +padding, off_d* = -dilation.
 * Cin % 32 == 0, in_ld % 4 == 0; bias nullable.  prof_tag: DIGA_PROF_CONV_FWD or DIGA_PROF_CONV_BWD_DATA. */
int diga_conv2d_nhwc_f32(const float* in, const float* wgt, const float* bias, float* out,
                         int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t in_ld,
                         int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                         int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                         int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag, void* stream);

/* stats_partial (nullable, diga_conv2d_stats_floats(N,Ho,Wo,Cout) floats): the epilogue also writes, per 128-pixel
 * tile and channel, sum(y - s), sum((y - s)^2), s -- the column-statistics partials of the BatchNorm that follows the
 * conv (diga_bn_fwd_partials), which then needs no statistics pass of its own over y. */
size_t diga_conv2d_stats_floats(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout);
/* Rows per statistics chunk the forward entry point will use for this layer: 128, or 64 where an fp32 stride-1 pointwise layer
 * runs on the persistent GEMM (each wave reduces its own 64 rows in registers).  Pass it to diga_bn_fwd_partials as chunk_rows;
 * diga_conv2d_stats_floats sizes the buffer for either. */
int diga_conv2d_stats_chunk_rows(int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t R,
                                 int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int math);
/* ... and of the `partials` records a backward-data epilogue (`_epi` entry points) will write for this geometry. */
int diga_conv2d_epi_chunk_rows(int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t R,
                               int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int math);

/* ------------------------------------------------------------------------------------
 * Backward-data with a fused epilogue.  The gradient a backward-data convolution produces is the input gradient of the
 * layer in front of it -- in the DeepLab trunk always a train-mode BatchNorm (+ReLU, + the residual junction of
 * G5/model/seg_model_noaux.py:81-101).  The `_epi` forms of the three convolution entry points finish that tensor on its
 * way out of the matrix cores instead of in separate passes over HBM:
 *     out = acc                               the convolution (bias-free, no forward statistics)
 *     out += addend                           the gradient reaching the same tensor through the residual branch
 *     out  = out where (mask_y > 0)           ReLU of a BatchNorm with residual (mask_y = its output)          -- or --
 *     out  = out where bit c of mask_bits     the same mask as one bit per channel (relu_bits of diga_bn_fwd*) -- or --
 *     out  = out where fma(x, a, b) > 0       ReLU of a BatchNorm without residual (relu_ab = its forward coefficients)
 *     partials[chunk] = { sum out, sum out*xhat } per 128-row chunk and channel, xhat = (x - mean) * invstd
 * `out` is then the MASKED gradient g of that BatchNorm and `partials` what diga_bn_bwd_partials finalises -- its
 * reduce pass over (g, x), the separate add and the residual-gradient copy are gone.  All tensors [M][ld] fp32 with
 * M = N*Ho*Wo rows, ld % 4 == 0, 16-byte aligned; Cout % 4 == 0; partials holds ceil(M/64)*2*Cout floats, of which the first
 * ceil(M/128)*2*Cout are written: one {sum, sum*xhat} record per chunk of diga_conv2d_epi_chunk_rows(...) rows -- 128 for every
 * shape and arithmetic (a call with an epilogue never runs on the persistent fp32 GEMM) -- pass that chunk size to
 * diga_bn_bwd_partials.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    const float* addend;   /* nullable */
    int64_t addend_ld;
    const float* mask_y;   /* nullable */
    int64_t mask_ld;
    const float* x;        /* nullable (needed by relu_ab and partials) */
    int64_t x_ld;
    const float* relu_ab;  /* nullable [2][Cout] */
    const float* mean;     /* [Cout] (with partials) */
    const float* invstd;   /* [Cout] (with partials) */
    float* partials;       /* nullable */
    const unsigned char* mask_bits;   /* nullable: [M][mask_bits_ld bytes], bit (c & 7) of byte (c >> 3) = keep channel c */
    int64_t mask_bits_ld;
} diga_bwd_epilogue_t;

int diga_conv2d_nhwc_f32_epi(const float* in, const float* wgt, float* out, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin,
                             int64_t in_ld, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                             int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy,
                             int64_t off_dx, const diga_bwd_epilogue_t* epi, int prof_tag, void* stream);
int diga_conv2d_nhwc_bf16x3_epi(const float* in, const uint16_t* wgt_hi, const uint16_t* wgt_lo, float* out, int64_t N,
                                int64_t Hi, int64_t Wi, int64_t Cin, int64_t in_ld, int64_t Ho, int64_t Wo, int64_t Cout,
                                int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                int64_t off_x0, int64_t off_dy, int64_t off_dx, const diga_bwd_epilogue_t* epi, int prof_tag,
                                void* stream);
int diga_conv2d_nhwc_twin_epi(const void* in_twin, const void* wgt_img, float* out, int64_t N, int64_t Hi, int64_t Wi,
                              int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                              int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy,
                              int64_t off_dx, const diga_bwd_epilogue_t* epi, int prof_tag, void* stream);

/* ------------------------------------------------------------------------------------
 * Forward with a fused INFERENCE epilogue: an eval-mode BatchNorm (running statistics: its a, b are constants of the checkpoint),
 * the residual add and the ReLU behind a convolution applied to the accumulators on their way out, instead of the conv storing its
 * raw output and diga_bn_fwd(training = 0) reading it back (one launch and two or three passes over the tensor per BatchNorm).
 * Per element, in this order:  v = acc;  v += bias (where a bias is given, as the plain entry points add it);
 * v = fma(v, a[c], b[c]);  v += residual;  v = fmaxf(v, 0) -- the expressions of the plain forward followed by diga_bn_fwd's apply
 * pass on the stored fp32 value, so the result is bit-identical to that pair of calls with ab = diga_bn_eval_coefficients(...).
 * The exact-fp32 kernels (the direct / LDS-DMA / persistent-GEMM kernels and the Winograd output transform of 4x4 / 6x6 tiles) and
 * the bf16x6 kernels (diga_infer_conv2d_nhwc_bf16x6 / _f32in, diga_infer_conv2d_winograd_bf16x6 below) have it; bf16x3 has not.
 * Cout % 4 == 0, out_ld % 4 == 0, residual_ld % 4 == 0 and >= Cout, all pointers 16-byte aligned, ab non-null; the residual may
 * alias nothing the kernel writes; no statistics output.  Anything else: DIGA_EINVAL.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    const float* ab;        /* [2][Cout]: a then b, 16-byte aligned -- y = fma(acc (+ bias), a, b) */
    const float* residual;  /* nullable [M][residual_ld], added after the fma */
    int64_t residual_ld;
    int relu;               /* fmaxf(., 0) last */
} diga_infer_epilogue_t;

/* diga_conv2d_nhwc_f32 without stats_partial, with the inference epilogue (non-null). */
int diga_conv2d_nhwc_f32_infer(const float* in, const float* wgt, const float* bias, float* out,
                               int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t in_ld,
                               int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                               int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                               int64_t off_dy, int64_t off_dx, const diga_infer_epilogue_t* infer, int prof_tag, void* stream);

/* Options of ONE forward convolution call (the `_opts` entry points below) -- the non-conv ops around the translator's
 * convolutions (G5/model/model_util.py:21-61: ReflectionPad2d -> Conv2d -> [norm] -> [activation];
 * G5/model/model_noaux.py:100-117: nn.Upsample(scale_factor=2) in front of a block) folded into the kernel's addressing
 * instead of separate passes over HBM:
 *   reflect_pad     1: taps outside the image read the mirrored pixel (index -i -> i, H-1+i -> H-1-i) instead of zero
 *   upsample_shift  s: the conv reads the 2^s nearest-neighbour upsampling of `in` ([N,Hi,Wi,Cin] stays the SOURCE tensor;
 *                      Ho/Wo and the tap offsets are those of the upsampled image)
 *   activation      1: tanh on the (biased) output
 * Passed explicitly with the call; the library keeps no per-thread or per-process mode.  Not combinable with BatchNorm
 * statistics output or a backward epilogue. */
typedef struct diga_conv_options {
    int reflect_pad;
    int upsample_shift;
    int activation;
} diga_conv_options_t;

/* Conv arithmetic.  The exact-fp32 and the split-bf16 kernels are SEPARATE entry points (diga_conv2d_nhwc_f32 vs
 * diga_conv2d_nhwc_bf16x3 / _twin); the one entry point that serves both, diga_conv2d_wgrad_nhwc_f32, takes the arithmetic
 * as an argument.  Which one a model runs in is host-side policy (diga_amd/_lib.py: set_conv_math, default from the
 * environment variable DIGA_CONV_MATH) -- the library holds no process-wide mode.
 *   DIGA_CONV_MATH_F32    v_mfma_f32_32x32x2_f32, exact fp32 (k-ordered fmaf chain)
 *   DIGA_CONV_MATH_BF16X3 operands split into bf16 hi+lo, hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with fp32
 *                         accumulate (~1e-5 relative per product)
 *   DIGA_CONV_MATH_BF16X6 operands carried exactly as THREE bf16 planes (24 significand bits), six of the nine plane products
 *                         on v_mfma_f32_16x16x32_bf16 with fp32 accumulate: fp32-equivalent (dropped terms <= 2^-24 of a
 *                         product).  Pointwise (1x1) layers only, through the diga_*_bf16x6 entry points below; the host runs
 *                         every other layer exactly as in DIGA_CONV_MATH_F32.  diga_conv2d_wgrad_nhwc_f32 does not take it. */
#define DIGA_CONV_MATH_F32 0
#define DIGA_CONV_MATH_BF16X3 1
#define DIGA_CONV_MATH_BF16X6 2

/* Tuned split-bf16 forward / backward-data: same contract as diga_conv2d_nhwc_f32 in DIGA_CONV_MATH_BF16X3, but the
 * weights are passed already split (diga_split_bf16 of the [Cout][R][S][Cin] array, once per step), so the kernel
 * stages them without arithmetic.  hi/lo are bf16 bit patterns; n % 4 == 0. */
int diga_split_bf16(const float* x, uint16_t* hi, uint16_t* lo, int64_t n, void* stream);
int diga_conv2d_nhwc_bf16x3(const float* in, const uint16_t* wgt_hi, const uint16_t* wgt_lo, const float* bias, float* out,
                            int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t in_ld,
                            int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                            int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                            int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag, void* stream);

/* The same convolution with BOTH operands pre-split and staged global -> LDS by LDS-DMA loads (no registers, no split
 * arithmetic, no ds_write in the kernel; three-stage LDS ring, one barrier per K-step; multi-tap layers run with two
 * MFMA waves per SIMD and skip the K-steps of taps that lie outside the image for a whole tile):
 *   in_twin  = diga_make_twin of the [N,Hi,Wi,Cin] fp32 activations: per pixel and group of 8 channels 16 B of bf16 hi
 *              + 16 B of bf16 lo (4*Cin bytes per pixel, dense);
 *   wgt_img  = diga_split_bf16_image of the [Cout][R][S][Cin] weights (diga_split_bf16_image_bytes bytes): the hi / lo
 *              LDS images of every (output-channel tile, K-step).
 * Cin % 32 == 0.  Pays when the activation tensor is read by many tiles (3x3 taps, wide Cout, several convs on one
 * input): the twin costs one extra pass (read 4 B + write 4 B per element). */
int diga_make_twin(const float* x, int64_t ld, void* twin, int64_t M, int64_t C, void* stream);
size_t diga_split_bf16_image_bytes(int64_t Cout, int64_t RS, int64_t Cin);
int diga_split_bf16_image(const float* w, void* img, int64_t Cout, int64_t RS, int64_t Cin, void* stream);
int diga_conv2d_nhwc_twin(const void* in_twin, const void* wgt_img, const float* bias, float* out, int64_t N, int64_t Hi,
                          int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                          int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                          float* stats_partial, int prof_tag, void* stream);

/* Winograd in fp32 for a stride-1 3x3 convolution with padding = dilation (output H x W = input H x W): same result as
 * diga_conv2d_nhwc_f32 with R = S = 3, offsets (-dilation, +dilation) up to fp32 rounding.
 *   tile = 2: F(2x2,3x3), 16 instead of 36 multiplications per 2x2 outputs, transforms with coefficients 0, +-1, +-1/2
 *             (as accurate as the direct fmaf chain);
 *   tile = 4: F(4x4,3x3), 36 instead of 144 multiplications per 4x4 outputs, points 0, +-1, +-2, inf (rounding error about
 *             10x the direct kernel's: max 1e-5 of the output scale on a 256-channel layer) -- the choice for the
 *             dilation 1 / 2 / 4 layers, whose d*d sub-images are large against a 4x4 tile.
 * The caller picks `tile` per call (every entry point of one layer -- workspace queries, forward, kept V, weight gradient --
 * must be given the same value); the library keeps no mode.  flip = 1 reads the taps in reverse order
 * (w[2-r][2-s]): with wgt = the [Cin][3][3][Cout] transpose this is the backward-data convolution.  No statistics / backward
 * epilogue.  Cin % 32 == 0, Cout % 4 == 0, Cout > 64.  Replaces the cuDNN call behind nn.Conv2d(3x3, dilation = padding) of
 * G5/model/seg_model_noaux.py:66-70,143-150,166-170.  workspace: diga_conv2d_winograd_workspace_bytes (16-byte aligned). */
size_t diga_conv2d_winograd_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t dilation, int64_t tile);
/* Round 5, two optional arguments of every Winograd entry point:
 *   tile_table (nullable): the layer's tile table -- a function of (N, H, W, dilation, tile) only -- built ONCE by
 *     diga_conv2d_winograd_tile_table into a caller-owned buffer of diga_conv2d_winograd_tile_table_bytes bytes and reused by every
 *     call on that geometry (forward, backward-data, backward-weight of all layers that share it); NULL: the call builds it in its
 *     workspace, one more launch (136 per C2 step before).
 *   stats_partial (nullable; forward of 4x4 / 6x6 tiles only): diga_conv2d_winograd_stats_floats floats; the output transform then
 *     also leaves the BatchNorm behind the layer its column statistics as diga_conv2d_winograd_stats_records RECORDS of unequal
 *     size -- [R][3][Cout] {sum (y - s), sum (y - s)^2, s} followed by [R] pixel counts -- for diga_bn_fwd_records
 *     (counts = stats_partial + R * 3 * Cout): no statistics pass over y. */
size_t diga_conv2d_winograd_tile_table_bytes(int64_t N, int64_t H, int64_t W, int64_t dilation, int64_t tile);
int diga_conv2d_winograd_tile_table(void* table, int64_t N, int64_t H, int64_t W, int64_t dilation, int64_t tile, void* stream);
size_t diga_conv2d_winograd_stats_records(int64_t N, int64_t H, int64_t W, int64_t Cout, int64_t dilation, int64_t tile);
size_t diga_conv2d_winograd_stats_floats(int64_t N, int64_t H, int64_t W, int64_t Cout, int64_t dilation, int64_t tile);
int diga_conv2d_winograd_f32(const float* in, const float* wgt, const float* bias, float* out, void* workspace,
                             size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t in_ld, int64_t Cout,
                             int64_t out_ld, int64_t dilation, int64_t tile, int flip, float* stats_partial, const void* tile_table,
                             int prof_tag, void* stream);
/* Forward with a diga_conv_options_t (inference-only, as the `_opts` forms of the direct kernels): reflect_pad folds
 * nn.ReflectionPad2d(dilation) into the input transform's tap addressing (the translator's 3x3 ResBlock convs,
 * G5/model/model_util.py:21-61: 54 % of its FLOPs); upsample_shift / activation must be 0 here (direct kernels).  tile = 4 or 6. */
int diga_conv2d_winograd_f32_opts(const float* in, const float* wgt, const float* bias, float* out, void* workspace,
                                  size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t in_ld, int64_t Cout,
                                  int64_t out_ld, int64_t dilation, int64_t tile, const diga_conv_options_t* opts, const void* tile_table,
                                  int prof_tag, void* stream);
/* ... with the backward-data epilogue of diga_bwd_epilogue_t (declared above; same arithmetic per element as the `_epi` forms
 * of the direct kernels; `partials` rows are filled per group of tiles instead of per 128 pixel rows -- the finaliser
 * diga_bn_bwd_partials only adds the rows up). */
int diga_conv2d_winograd_f32_epi(const float* in, const float* wgt, float* out, void* workspace, size_t workspace_bytes, int64_t N,
                                 int64_t H, int64_t W, int64_t Cin, int64_t in_ld, int64_t Cout, int64_t out_ld, int64_t dilation,
                                 int64_t tile, int flip, const diga_bwd_epilogue_t* epi, const void* tile_table, int prof_tag,
                                 void* stream);
/* Forward (flip = 0, no statistics) with the inference epilogue of diga_infer_epilogue_t in the output transform; tile = 4 or 6
 * (tile 2: DIGA_EINVAL -- the caller runs the plain forward and diga_bn_fwd there). */
int diga_conv2d_winograd_f32_infer(const float* in, const float* wgt, const float* bias, float* out, void* workspace,
                                   size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t in_ld, int64_t Cout,
                                   int64_t out_ld, int64_t dilation, int64_t tile, const diga_infer_epilogue_t* infer,
                                   const void* tile_table, int prof_tag, void* stream);
/* Backward-weight of the same layer through Winograd (dw [Cout][3][3][Cin] = G^T [sum over tiles (A dY A^T) (.) (B^T d B)] G):
 * transforms of dy and x, the 16 (tile 2) / 36 (tile 4) products contracted over the tiles in one launch of the fp32 LDS-DMA
 * backward-weight kernel (fixed-order split-K: bit-reproducible), the transform back to 3x3.  Cout % 256 == 0, Cin % 128 == 0. */
size_t diga_conv2d_wgrad_winograd_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t dilation,
                                                  int64_t tile, int v_kept /* 1: the call will pass the forward's kept V */);
int diga_conv2d_wgrad_winograd_f32(const float* dy, const float* x, const float* v_kept, float* dw, void* workspace,
                                   size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t x_ld, int64_t Cout,
                                   int64_t dy_ld, int64_t dilation, int64_t tile, const void* tile_table, void* stream);
/* Forward that leaves its transformed input V (diga_conv2d_winograd_v_floats floats, 4x the input tensor) in `v_keep` for the
 * weight gradient of the same layer: pass it as `v_kept` above (x may then be null) and the backward skips the input transform
 * -- HBM is 288 GB: the transform is a bandwidth pass of 5x the input's bytes per 3x3 layer. */
size_t diga_conv2d_winograd_v_floats(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t dilation, int64_t tile);
int diga_conv2d_winograd_f32_keep(const float* in, const float* wgt, const float* bias, float* out, float* v_keep, void* workspace,
                                  size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t in_ld, int64_t Cout,
                                  int64_t out_ld, int64_t dilation, int64_t tile, float* stats_partial, const void* tile_table, int prof_tag,
                                  void* stream);

/* diga_conv2d_nhwc_f32 / _bf16x3 / _twin with a diga_conv_options_t (non-null; inference-only: no statistics output). */
int diga_conv2d_nhwc_f32_opts(const float* in, const float* wgt, const float* bias, float* out, int64_t N, int64_t Hi, int64_t Wi,
                              int64_t Cin, int64_t in_ld, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                              int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                              const diga_conv_options_t* opts, int prof_tag, void* stream);
int diga_conv2d_nhwc_bf16x3_opts(const float* in, const uint16_t* wgt_hi, const uint16_t* wgt_lo, const float* bias, float* out,
                                 int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t in_ld, int64_t Ho, int64_t Wo, int64_t Cout,
                                 int64_t out_ld, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                 int64_t off_x0, int64_t off_dy, int64_t off_dx, const diga_conv_options_t* opts, int prof_tag,
                                 void* stream);
int diga_conv2d_nhwc_twin_opts(const void* in_twin, const void* wgt_img, const float* bias, float* out, int64_t N, int64_t Hi,
                               int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                               int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                               const diga_conv_options_t* opts, int prof_tag, void* stream);

/* dw[k][r][s][c] = sum_{n,ho,wo} dy[n,ho,wo,k] * x[n, ho*stride_y + off_y0 + r*off_dy, wo*stride_x + off_x0 + s*off_dx, c]
 * Split over pixel ranges into fp32 slabs in `workspace`, summed in fixed order (deterministic).
 * math = DIGA_CONV_MATH_F32 (exact fp32 MFMA) or DIGA_CONV_MATH_BF16X3 (operands split in the kernel).  Cin % 4 == 0,
 * Cout % 4 == 0. */
size_t diga_conv2d_wgrad_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin,
                                         int64_t R, int64_t S);
int diga_conv2d_wgrad_nhwc_f32(const float* dy, const float* x, float* dw, void* workspace, size_t workspace_bytes,
                               int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t x_ld,
                               int64_t Ho, int64_t Wo, int64_t Cout, int64_t dy_ld, int64_t R, int64_t S,
                               int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                               int64_t off_dy, int64_t off_dx, int math, void* stream);

/* Backward-weight of the same convolution on the split twins (diga_make_twin of dy [N,Ho,Wo,Cout] and of x
 * [N,Hi,Wi,Cin], both dense): operands staged by LDS-DMA, fragments read with transposing LDS reads.  dw [Cout][R][S][Cin].
 * Pays where the twins exist anyway (multi-tap layers: x twin from the forward pass, dy twin from backward-data). */
size_t diga_conv2d_wgrad_twin_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R, int64_t S);
int diga_conv2d_wgrad_twin(const void* dy_twin, const void* x_twin, float* dw, void* workspace, size_t workspace_bytes,
                           int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t R,
                           int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy,
                           int64_t off_dx, void* stream);

/* bf16x6 (DIGA_CONV_MATH_BF16X6): 1x1 convolutions with BOTH operands pre-split into three bf16 planes and staged by LDS-DMA.
 *   triplet  = diga_make_triplet of dense [M][C] fp32 activations (C % 8 == 0): per pixel and group of 8 channels 16 B of
 *              plane 0, 16 B of plane 1, 16 B of plane 2, plane0 = bf16(a), plane1 = bf16(a - plane0), plane2 =
 *              bf16(a - plane0 - plane1) (6*C bytes per pixel; the planes sum to a exactly for normal fp32 of magnitude
 *              >= 2^-110; a non-finite a gives nan in the low planes);
 *   wgt_img  = diga_split_bf16x6_image of the [Cout][R*S][Cin] weights (diga_split_bf16x6_image_bytes bytes, Cin % 32 == 0):
 *              the three planes as LDS images per (output-channel tile, 32-channel K-step).
 * Per product a1 b1 + a0 b2 + a2 b0 + a0 b1 + a1 b0 + a0 b0, fp32 accumulate, the five small terms summed apart per
 * 32-deep K-step.  diga_conv2d_nhwc_bf16x6 / _epi: the contract of diga_conv2d_nhwc_twin / _twin_epi (bias, stats_partial
 * in 128-row chunks, the diga_bwd_epilogue_t epilogue) restricted to R == S == 1 (any stride / offset: pixels outside the
 * image read zeros).  diga_conv2d_wgrad_bf16x6: dw [Cout][Cin] from the triplets of dy [N,Ho,Wo,Cout] and x [N,Hi,Wi,Cin]
 * (channel counts % 8 == 0), split over pixel ranges and summed in fixed order (deterministic); workspace 16-byte aligned. */
int diga_make_triplet(const float* x, int64_t ld, void* triplet, int64_t M, int64_t C, void* stream);
size_t diga_split_bf16x6_image_bytes(int64_t Cout, int64_t RS, int64_t Cin);
int diga_split_bf16x6_image(const float* w, void* img, int64_t Cout, int64_t RS, int64_t Cin, void* stream);
int diga_conv2d_nhwc_bf16x6(const void* in_triplet, const void* wgt_img, const float* bias, float* out, int64_t N, int64_t Hi,
                            int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                            int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                            float* stats_partial, int prof_tag, void* stream);
int diga_conv2d_nhwc_bf16x6_epi(const void* in_triplet, const void* wgt_img, float* out, int64_t N, int64_t Hi, int64_t Wi,
                                int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                                int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                                const diga_bwd_epilogue_t* epi, int prof_tag, void* stream);
size_t diga_conv2d_wgrad_bf16x6_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R, int64_t S);
int diga_conv2d_wgrad_bf16x6(const void* dy_triplet, const void* x_triplet, float* dw, void* workspace, size_t workspace_bytes,
                             int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t R,
                             int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy,
                             int64_t off_dx, void* stream);

/* bf16x6 straight from fp32 tensors ("loader split"): the same kernels with the three-plane split done by their loader waves on
 * the way into LDS -- no diga_make_triplet pass, no triplet buffer, and the operands may be channel slices of wider NHWC buffers.
 * `in` / `dy` / `x` are fp32 [pixel][ld] with ld >= the channel count, ld % 4 == 0 (else DIGA_EINVAL) and 16-byte aligned base
 * pointers (else DIGA_EALIGN); wgt_img, bias, stats_partial, epi, the geometry, the channel-count rules (forward Cin % 32 == 0,
 * weight gradient Cin % 8 == 0 and Cout % 8 == 0) and the workspace (diga_conv2d_wgrad_bf16x6_workspace_bytes) are those of the
 * triplet forms above.  The planes and the order of the products are the same: results are bit-identical to diga_make_triplet
 * followed by the triplet form. */
int diga_conv2d_nhwc_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N,
                                  int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                  int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                  int64_t off_dy, int64_t off_dx, float* stats_partial, int prof_tag, void* stream);
int diga_conv2d_nhwc_bf16x6_f32in_epi(const float* in, int64_t in_ld, const void* wgt_img, float* out, int64_t N, int64_t Hi,
                                      int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R,
                                      int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy,
                                      int64_t off_dx, const diga_bwd_epilogue_t* epi, int prof_tag, void* stream);
int diga_conv2d_wgrad_bf16x6_f32in(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw, void* workspace,
                                   size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo,
                                   int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                   int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream);

/* The two forward forms above without stats_partial, with the inference epilogue of diga_infer_epilogue_t (non-null) applied to the
 * staged accumulator tile on its way out: the K loop is the plain entry point's, so the result is bit-identical to
 * diga_conv2d_nhwc_bf16x6 / _f32in followed by diga_bn_fwd(training = 0).  The rules are those of diga_conv2d_nhwc_f32_infer: Cout % 4
 * == 0, out_ld % 4 == 0, residual_ld % 4 == 0 and >= Cout, `out`, `bias`, `ab` and the residual 16-byte aligned, ab non-null, forward
 * only (else DIGA_EINVAL); every check precedes the launch.  (Named diga_infer_*: the diga_conv2d_* names are the ones the dispatch
 * fixture of the test suite enumerates, and that fixture records training and fp32 scenarios only.) */
int diga_infer_conv2d_nhwc_bf16x6(const void* in_triplet, const void* wgt_img, const float* bias, float* out, int64_t N, int64_t Hi,
                                  int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                                  int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                                  const diga_infer_epilogue_t* infer, int prof_tag, void* stream);
int diga_infer_conv2d_nhwc_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N,
                                        int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                        int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                        int64_t off_dy, int64_t off_dx, const diga_infer_epilogue_t* infer, int prof_tag,
                                        void* stream);

/* bf16x6 for convolutions with more than one tap (opt-in: StepConfig.x6_taps under conv_math = 2), loader form only: `in` / `dy` / `x`
 * are the fp32 tensors, the weights the tap-major image of diga_split_bf16x6_image(w [Cout][R*S][Cin], ..., Cout, R * S, Cin).  The
 * argument lists are those of the pointwise `_f32in` entry points above; the taps sit at (off_y0 + r * off_dy, off_x0 + s * off_dx),
 * either sign (backward-data passes the negated offsets and the transposed weights), any stride; a tap outside the image reads zeros.
 * The K loop walks the taps in the image's order and steps over those that lie outside the image for a block's whole row tile, so the
 * result is, bit for bit, diga_conv2d_nhwc_bf16x6_f32in on the tap-major im2col rows [M][R*S*Cin]; R = S = 1 gives the pointwise
 * kernel's bits.  Checked before any launch: non-null 16-byte aligned pointers, Cin % 32 == 0, in_ld / out_ld, 1 <= R * S <= 64,
 * positive strides, pixel counts and pixel coordinates below 2^31, the epilogue descriptors' rules (DIGA_EINVAL / DIGA_EALIGN).
 * (Not named diga_conv2d_*: see diga_infer_conv2d_nhwc_bf16x6.) */
int diga_conv_taps_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N, int64_t Hi,
                                int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                                int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                                float* stats_partial, int prof_tag, void* stream);
int diga_conv_taps_bf16x6_f32in_epi(const float* in, int64_t in_ld, const void* wgt_img, float* out, int64_t N, int64_t Hi, int64_t Wi,
                                    int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R, int64_t S,
                                    int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0, int64_t off_dy, int64_t off_dx,
                                    const diga_bwd_epilogue_t* epi, int prof_tag, void* stream);
int diga_infer_conv_taps_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N,
                                      int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                      int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                      int64_t off_dy, int64_t off_dx, const diga_infer_epilogue_t* infer, int prof_tag, void* stream);
/* diga_conv_taps_bf16x6_f32in with a diga_conv_options_t (non-null, else DIGA_EINVAL; opt-in: StepConfig.x6_opts next to x6_taps):
 * its argument list plus `opts` behind stats_partial.  `in` is the SOURCE tensor [N][Hi][Wi]; the loader waves map every tap's
 * coordinate -- in the image upsampled by 2^upsample_shift -- to its source pixel: mirrored at both borders under reflect_pad, zeros
 * outside without it; activation 1 is tanh on the output (the direct `_opts` kernels' drain).  Weight image, K-step order, MFMA
 * sequence and drain are diga_conv_taps_bf16x6_f32in's: the result is, bit for bit, that entry point on the explicitly upsampled and
 * padded image.  Inference-only: stats_partial must be null and there is no epilogue form; the options' rules are those of
 * diga_conv2d_nhwc_f32_opts (reflect_pad 0/1, upsample_shift 0..2, activation 0/1); Hi << upsample_shift and Wi << upsample_shift
 * stay below 2^30; every other check as above. */
int diga_conv_taps_bf16x6_f32in_opts(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N,
                                     int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld,
                                     int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0, int64_t off_x0,
                                     int64_t off_dy, int64_t off_dx, float* stats_partial /* null */, const diga_conv_options_t* opts,
                                     int prof_tag, void* stream);
/* The "window form" of the multi-tap forward (opt-in: StepConfig.x6_window next to x6_taps under conv_math = 2): for convolutions of
 * stride 1 in the logical image (`in` upsampled by 2^upsample_shift, before padding) a block owns th x tw output pixels of one image
 * and splits their input window -- (th + (R - 1) dil_y) x (tw + (S - 1) dil_x) logical pixels of one 32-channel chunk, every pixel
 * through the `_opts` form's map (mirror, clamp, shift to the source pixel; zero planes and no load for zero padding) -- into LDS
 * once; all R * S taps are walked from there.  K-steps run chunk-major: at Cin == 32 the result is, bit for bit,
 * diga_conv_taps_bf16x6_f32in[_opts]'s; at Cin > 32 the same products are summed chunk by chunk (same error level).  Cout > 64 runs
 * ceil(Cout / 64) column tiles, each splitting the window again.
 *
 * diga_conv_window_bf16x6_plan: a pure query, the one statement of the rule.  Returns 1 and *th, *tw (th * tw % 128 == 0; 8 x 16)
 *   and *cols (16 for Cout <= 16, else 64) where the window form takes the call, 0 (nothing written) where it does not: Cin not a
 *   positive multiple of 32, R * S outside 2 .. 64, a dilation below 1, upsample_shift outside 0 .. 2, null pointers, or a window
 *   that does not fit: 2 * 3 * cols * 64 (weight ring) + max(window pixels * 192, th * tw * (cols + 4) * 4) > 160 KB.
 * diga_conv_window_bf16x6_f32in: taps at (off_y0 + r * dil_y, off_x0 + q * dil_x), stride 1; `opts` nullable (its rules as above);
 *   bias and tanh as in the `_opts` form, no statistics, no epilogue.  DIGA_EINVAL for everything the rule refuses, for in_ld < Cin
 *   or in_ld % 4 != 0, out_ld < Cout, and for reflection padding not smaller than the logical extent; DIGA_EALIGN for `in` / `wgt_img`
 *   off 16 bytes or `out` / `bias` off 4.  The weight image is diga_split_bf16x6_image's. */
int diga_conv_window_bf16x6_plan(int64_t Hi, int64_t Wi, int64_t Cin, int64_t Cout, int64_t R, int64_t S, int64_t dil_y, int64_t dil_x,
                                 int64_t upsample_shift, int* th, int* tw, int* cols);
int diga_conv_window_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const float* bias, float* out, int64_t N,
                                  int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t out_ld, int64_t R,
                                  int64_t S, int64_t off_y0, int64_t off_x0, int64_t dil_y, int64_t dil_x,
                                  const diga_conv_options_t* opts /* nullable */, int prof_tag, void* stream);
/* The window form of a 2x nearest-upsampled input on PHASE-COLLAPSED weights (opt-in: StepConfig.x6_up2 next to x6_taps, x6_opts and
 * x6_window under conv_math = 2).  After nearest x2 upsampling output pixel (2 y + fy, 2 x + fx) reads, for tap r, source row
 * y + a(fy, r) with a(f, r) = floor((f + off_y0 + r) / 2) (columns alike): away from the padding the layer is four stride-1
 * convolutions of the SOURCE image, one per output phase (fy, fx), each with R' x S' taps that are sums of the layer's -- collapsed tap
 * index a(f, r) - a(f, 0), R' = max over f of a(f, R - 1) - a(f, 0) + 1 (5 x 5 at pad 2: 3 x 3).  At the padding no collapsed weight
 * reproduces the layer, so the 8 x 16 tiles of the window form are split: the INTERIOR tiles (1 <= by <= tiles_y - 2,
 * 1 <= bx <= tiles_x - 2) run on the collapsed weights (conv_up2_x6_kernel), the ring of border tiles on the window walk with the
 * layer's own image -- bit for bit what diga_conv_window_bf16x6_f32in gives those tiles.  An interior pixel is, bit for bit, the window
 * form's result for its phase's collapsed weights on the source image.
 *
 * diga_conv_up2_bf16x6_plan: a pure query, the one statement of the rule.  Returns 1 and *rc = R', *sc = S' where the form takes the
 *   call, 0 (nothing written) where it does not: whatever diga_conv_window_bf16x6_plan refuses or gives 16 columns (Cout <= 16),
 *   upsample_shift != 1, a dilation other than 1, R or S outside 2 .. 7, off_y0 or off_x0 > 0, reflect_pad outside 0 / 1, fewer than
 *   3 x 3 tiles, an interior tap outside the logical image [0, 2 Hi) x [0, 2 Wi), null pointers.
 * diga_collapse_up2_weights: w_krsc [K][R][S][C] -> wc [fy][fx][K][R'][S'][C] fp32; each element the sum of its group taken in double in
 *   ascending (r, s) order and rounded once; a phase with fewer taps keeps zeros in the rest.  DIGA_EINVAL for R, S outside 2 .. 7 or
 *   positive offsets, DIGA_EALIGN for pointers off 16 bytes.
 * diga_conv_up2_bf16x6_f32in: diga_conv_window_bf16x6_f32in's arguments at unit dilation with a non-null `opts` (upsample_shift = 1) and
 *   wgt_img_phases = diga_split_bf16x6_image of the four [K][R'][S'][C] tensors, consecutive
 *   (diga_split_bf16x6_image_bytes(Cout, R' * S', Cin) apart); wgt_img stays the layer's own image.  Two launches on the stream that
 *   write disjoint pixels.  Refusals as diga_conv_window_bf16x6_f32in's, plus everything the rule refuses. */
int diga_conv_up2_bf16x6_plan(int64_t Hi, int64_t Wi, int64_t Cin, int64_t Cout, int64_t Ho, int64_t Wo, int64_t R, int64_t S,
                              int64_t off_y0, int64_t off_x0, int64_t dil_y, int64_t dil_x, int64_t upsample_shift, int64_t reflect_pad,
                              int* rc, int* sc);
int diga_collapse_up2_weights(const float* w_krsc, float* wc, int64_t K, int64_t R, int64_t S, int64_t C, int64_t off_y0, int64_t off_x0,
                              void* stream);
int diga_conv_up2_bf16x6_f32in(const float* in, int64_t in_ld, const void* wgt_img, const void* wgt_img_phases, const float* bias,
                               float* out, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout,
                               int64_t out_ld, int64_t R, int64_t S, int64_t off_y0, int64_t off_x0, const diga_conv_options_t* opts,
                               int prof_tag, void* stream);
/* ... and their weight gradient dw [Cout][R][S][Cin]: diga_conv2d_wgrad_bf16x6_f32in's arguments with 1 <= R * S <= 64, Cin % 32 == 0
 * and Cout % 8 == 0; one block group per tap, split-K by the bf16x6 plan with the taps counted among the tiles.  The workspace query
 * returns 0 for a shape the entry point rejects (DIGA_EINVAL); a workspace smaller than it asks for: DIGA_EWORKSPACE. */
size_t diga_conv_taps_wgrad_bf16x6_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R, int64_t S);
int diga_conv_taps_wgrad_bf16x6_f32in(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw, void* workspace,
                                      size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo,
                                      int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                      int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream);

/* The loader-form weight gradient on the tile that fits the layer (opt-in: StepConfig.x6_wgrad_tile = "fit" under conv_math = 2).
 * The two entry points above run one tile, 256 (Cout) x 128 (Cin); a narrow layer pays six MFMAs per product on the padding.
 *
 * diga_wgrad_bf16x6_tile: a pure query, the one statement of the tile rule.  *bm = 64 if Cout <= 64, 128 if Cout <= 128, else 256;
 *   *bn = 64 if Cin <= 64, else 128; (128, 64) is not built and answers (128, 128).  Non-positive or non-multiple-of-8 channel
 *   counts, null pointers: DIGA_EINVAL.
 * diga_wgrad_bf16x6_tiled_f32in: the argument list and checks of diga_conv_taps_wgrad_bf16x6_f32in with 1 <= R * S <= 64,
 *   Cin % 32 == 0 when R * S > 1, else Cin % 8 == 0, and Cout % 8 == 0.  A shape whose tile is (256, 128) runs exactly what
 *   diga_conv2d_wgrad_bf16x6_f32in (R * S = 1) / diga_conv_taps_wgrad_bf16x6_f32in run.  Any other tile runs the same arithmetic --
 *   product order, fold accumulator, clamps, slab layout, fixed-order reduce -- on its own split-K plan: at least 8 K-steps per
 *   block, at most 512 ranges, about two rounds of resident blocks (3 / 2 / 1 / 1 blocks per CU at 64x64 / 64x128 / 128x128 / 256x64).  Where both
 *   plans cut the pixels into the same ranges dw is bit-identical to the wide tile's; otherwise it is another split-K tree of the
 *   same error level.
 * diga_wgrad_bf16x6_tiled_workspace_bytes: its workspace; 0 for a shape the entry point rejects. */
int diga_wgrad_bf16x6_tile(int64_t Cout, int64_t Cin, int* bm, int* bn);
size_t diga_wgrad_bf16x6_tiled_workspace_bytes(int64_t N, int64_t Ho, int64_t Wo, int64_t Cout, int64_t Cin, int64_t R, int64_t S);
int diga_wgrad_bf16x6_tiled_f32in(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw, void* workspace,
                                  size_t workspace_bytes, int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo,
                                  int64_t Cout, int64_t R, int64_t S, int64_t stride_y, int64_t stride_x, int64_t off_y0,
                                  int64_t off_x0, int64_t off_dy, int64_t off_dx, void* stream);

/* bf16x6 for the Winograd-domain GEMMs of the stride-1 3x3 layers (opt-in: StepConfig.x6_winograd under conv_math = 2).  The
 * Winograd transforms stay fp32; the (tile + 2)^2 products per layer run on the loader-split bf16x6 kernels in ONE batched launch.
 *
 * diga_gemm_batched_bf16x6_f32in: out_b [rows x Cout] = A_b [rows x K] * W_b^T for b < batches.  A is [batches * rows_per_batch][K]
 *   fp32 (dense, read in place), out [batches * rows_per_batch][Cout]; wgt_imgs holds `batches` consecutive images of
 *   diga_split_bf16x6_image_bytes(Cout, 1, K) bytes, image b = diga_split_bf16x6_image(W_b [Cout][K], ..., Cout, 1, K).  A 256-row tile
 *   runs the K-steps of diga_conv2d_nhwc_bf16x6_f32in in the same order: each batch's block is bit-identical to that entry point on
 *   the batch alone.  rows_per_batch % 256 == 0, K % 32 == 0, Cout % 4 == 0 and Cout > 64, batches < 65536 (else DIGA_EINVAL);
 *   16-byte aligned pointers (else DIGA_EALIGN).  Index limits of the kernel: tile and row indices are 32-bit, so
 *   batches * rows_per_batch < 2^31 and (batches * rows_per_batch / 256) * ceil(Cout / 128) < 2^31 (else DIGA_EINVAL); element
 *   offsets are 64-bit.
 * diga_wgrad_batched_bf16x6_f32in: dU_b [Cout x Cin] = Z_b^T V_b (contraction over the rows).  Z [batches][rows][Cout],
 *   V [batches][rows][Cin] fp32 dense, dU [Cout][batches][Cin].  rows % 32 == 0, Cout % 256 == 0, Cin % 128 == 0, batches < 65536,
 *   rows < 2^31 and (Cout / 256) * (Cin / 128) * batches * splits < 2^31 blocks (else DIGA_EINVAL).  Split over row ranges of at
 *   least 8 K-steps (about two rounds of blocks), partial sums in `workspace` (diga_wgrad_batched_bf16x6_workspace_bytes; 0 for a
 *   rejected shape) added in fixed order: bit-reproducible.
 * diga_conv2d_winograd_bf16x6: diga_conv2d_winograd_f32 / _keep / _epi in one entry point with the products on the first GEMM:
 *   v_keep (nullable, forward only) as in `_keep`, stats_partial (nullable, tile 4 / 6, forward) as in `_f32`, epi (nullable) as in
 *   `_epi`; same tile table, transforms, shape rules (Cin % 32 == 0, Cout % 4 == 0 and > 64, leading dimensions % 4 == 0, tiles 2 / 4
 *   / 6) and the GEMM's index limits above on (tile + 2)^2 batches of the padded tile count.  Workspace
 *   (diga_conv2d_winograd_bf16x6_workspace_bytes; 0 for a rejected shape) = the fp32 form's + the weight images.
 * diga_conv_winograd_bf16x6_opts: diga_conv2d_winograd_f32_opts (same arguments and rules: non-null options of which only reflect_pad
 *   may be set, forward, no statistics, no epilogue, pad < H, W) on tiles of 4 or 6, with the products on the first GEMM and the
 *   workspace of diga_conv2d_winograd_bf16x6_workspace_bytes (opt-in: StepConfig.x6_opts next to x6_winograd).  The mirror lives in the
 *   input transform only; the GEMM and the output transform are diga_conv2d_winograd_bf16x6's.
 * diga_infer_conv2d_winograd_bf16x6: diga_conv2d_winograd_f32_infer (same arguments and rules: tile 4 or 6, forward, no statistics)
 *   with the products on the first GEMM and the workspace of diga_conv2d_winograd_bf16x6_workspace_bytes; bit-identical to
 *   diga_conv2d_winograd_bf16x6 followed by diga_bn_fwd(training = 0).
 * diga_conv2d_wgrad_winograd_bf16x6: diga_conv2d_wgrad_winograd_f32 (same arguments, Cout % 256 == 0, Cin % 128 == 0) with the
 *   products on the second GEMM; workspace diga_conv2d_wgrad_winograd_bf16x6_workspace_bytes. */
int diga_gemm_batched_bf16x6_f32in(const float* A, int64_t rows_per_batch, int64_t batches, int64_t K, const void* wgt_imgs,
                                   int64_t Cout, float* out, void* stream);
size_t diga_wgrad_batched_bf16x6_workspace_bytes(int64_t rows, int64_t batches, int64_t Cout, int64_t Cin);
int diga_wgrad_batched_bf16x6_f32in(const float* Z, const float* V, float* dU, void* workspace, size_t workspace_bytes, int64_t rows,
                                    int64_t batches, int64_t Cout, int64_t Cin, void* stream);
size_t diga_conv2d_winograd_bf16x6_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t dilation,
                                                   int64_t tile);
int diga_conv2d_winograd_bf16x6(const float* in, const float* wgt, const float* bias, float* out, float* v_keep /* nullable */,
                                void* workspace, size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t in_ld,
                                int64_t Cout, int64_t out_ld, int64_t dilation, int64_t tile, int flip,
                                float* stats_partial /* nullable */, const diga_bwd_epilogue_t* epi /* nullable */,
                                const void* tile_table, int prof_tag, void* stream);
int diga_infer_conv2d_winograd_bf16x6(const float* in, const float* wgt, const float* bias, float* out, void* workspace,
                                      size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t in_ld, int64_t Cout,
                                      int64_t out_ld, int64_t dilation, int64_t tile, const diga_infer_epilogue_t* infer,
                                      const void* tile_table, int prof_tag, void* stream);
int diga_conv_winograd_bf16x6_opts(const float* in, const float* wgt, const float* bias, float* out, void* workspace,
                                   size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t in_ld, int64_t Cout,
                                   int64_t out_ld, int64_t dilation, int64_t tile, const diga_conv_options_t* opts,
                                   const void* tile_table, int prof_tag, void* stream);
size_t diga_conv2d_wgrad_winograd_bf16x6_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t dilation,
                                                         int64_t tile, int v_kept);
int diga_conv2d_wgrad_winograd_bf16x6(const float* dy, const float* x, const float* v_kept, float* dw, void* workspace,
                                      size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t x_ld, int64_t Cout,
                                      int64_t dy_ld, int64_t dilation, int64_t tile, const void* tile_table, void* stream);

/* Stem (7x7/2 on the 3-channel NCHW image, G5/model/seg_model_noaux.py:221): out[n,ho,wo][(r*S+s)*C + c] =
 * x[n,c,ho*stride-pad+r,wo*stride-pad+s] (zero outside / beyond R*S*C up to Kpad), after which the conv is a
 * 1x1 conv with Cin = Kpad on the kernels above. */
int diga_im2col_nchw(const float* x, float* out, int64_t N, int64_t C, int64_t H, int64_t W, int64_t R, int64_t S,
                     int64_t stride, int64_t pad, int64_t Ho, int64_t Wo, int64_t Kpad, void* stream);

/* w [K][RS][C] -> wt [C][RS][K] (weights for backward-data). */
int diga_weight_transpose(const float* w, float* wt, int64_t K, int64_t RS, int64_t C, void* stream);

/* Backward-data of a stride-2 convolution (dilation 1, zero padding), exact fp32 under every diga_set_conv_math mode:
 *   dx[n, y, x, c] = sum_{r,s,k} dy[n, (y + pad_y - r)/2, (x + pad_x - s)/2, k] * wgt_t[c][r][s][k]
 * over the taps whose two quotients are exact and inside [0, Ho) x [0, Wo).  Hi, Wi, Cin, Ho, Wo, Cout, R, S name the FORWARD
 * convolution (x [N][Hi][Wi][Cin] -> y [N][Ho][Wo][Cout]); dy is [N][Ho][Wo][dy_ld], dx [N][Hi][Wi][dx_ld], wgt_t the
 * [Cin][R][S][Cout] transpose (diga_weight_transpose).  dx is split into its four phases (y & 1, x & 1); each is a stride-1
 * correlation of dy with the taps of its parity, read in place from wgt_t, so the call multiplies what the forward multiplies
 * (a quarter of the zero-insertion form) in one launch.  Every element of dx[.., :Cin] is written -- zeros where a phase has no
 * tap (R or S = 1, or 2 with one parity of the padding) and where no tap reaches (e.g. Hi = 8, R = 3, pad 0: row 7) -- so dx
 * may be uninitialised; channels Cin .. dx_ld are not touched.  Fixed summation order (tap-major, channel-minor): deterministic.
 * Rules, all DIGA_EINVAL and checked before the launch: non-null, 16-byte aligned pointers; dy_ld >= Cout, dx_ld >= Cin, both
 * % 4 == 0; Cout % 32 == 0, Cin % 4 == 0; stride_y == stride_x == 2; 1 <= R, S <= 7; 0 <= pad_y < R, 0 <= pad_x < S;
 * Ho == (Hi + 2 pad_y - R) / 2 + 1 >= 1 and Wo likewise; every phase's row count and all pixel coordinates below 2^30.
 * N == 0: DIGA_OK without a launch.  Profiling tag: DIGA_PROF_CONV_BWD_DATA. */
int diga_dgrad_strided_f32(const float* dy, int64_t dy_ld, const float* wgt_t /* [Cin][R][S][Cout] */, float* dx, int64_t dx_ld,
                           int64_t N, int64_t Hi, int64_t Wi, int64_t Cin, int64_t Ho, int64_t Wo, int64_t Cout, int64_t R, int64_t S,
                           int64_t stride_y, int64_t stride_x, int64_t pad_y, int64_t pad_x, void* stream);

/* ------------------------------------------------------------------------------------
 * Normalisation / pooling on NHWC fp32 (nn.BatchNorm2d with frozen affine in train mode, nn.GroupNorm(32),
 * SEBlock, nn.Dropout2d, nn.MaxPool2d(3,2,1,ceil_mode) of G5/model/seg_model_noaux.py:57-101,122-137,
 * 140-214,216-232).  x/y/... are [rows][C] with `ld_*` floats between rows; C % 4 == 0.
 * ---------------------------------------------------------------------------------- */
size_t diga_norm_workspace_bytes(int64_t rows_per_segment, int64_t n_segments, int64_t C);

/* y = [relu]( fma(x, a, b) [+ residual] ), a = invstd*gamma, b = beta - mean*a.  training: batch statistics over the
 * M rows (biased variance), running_mean/var updated with `momentum` (unbiased variance), statistics saved for the
 * backward pass; eval: running statistics.  residual nullable.  save_ab (nullable, [2][C]) receives a and b: passed
 * back to diga_bn_bwd as `relu_ab` it lets the backward of a residual-free BN+ReLU re-derive the ReLU mask from x
 * instead of reading y.  y_twin != 0: y (dense, ld_y == C, C % 8 == 0) receives the split twin of the result (the
 * format of diga_make_twin, 4 bytes per element) instead of fp32 -- for a tensor read only by the twin conv kernels.
 * relu_bits (nullable; relu, C % 32 == 0): also receives the ReLU mask as [M][C/8] bytes, bit (c & 7) of byte (c >> 3) =
 * (y[c] > 0) -- `mask_bits` of diga_bwd_epilogue_t: the backward-data epilogue of the conv that consumes y reads 1 bit
 * per element instead of y itself. */
int diga_bn_fwd(const float* x, int64_t ld_x, float* y, int64_t ld_y, const float* residual, int64_t ld_r,
                const float* gamma, const float* beta, float* running_mean, float* running_var,
                float* save_mean, float* save_invstd, float* save_ab, int64_t M, int64_t C, int training, int relu,
                int y_twin, unsigned char* relu_bits, float momentum, float eps, void* workspace, size_t workspace_bytes,
                void* stream);

/* The coefficients diga_bn_fwd(training = 0) applies: ab [2][C], a = gamma / sqrt(running_var + eps), b = beta - running_mean * a --
 * one launch of the very kernel diga_bn_fwd runs in eval mode, so that a caller of the `_infer` convolutions gets the same bits. */
int diga_bn_eval_coefficients(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                              float* ab, int64_t C, float eps, void* stream);

/* Train-mode diga_bn_fwd whose statistics pass is replaced by partials the producing conv already wrote
 * (`partial` = stats_partial of diga_conv2d_nhwc_*, `chunk_rows` = 128). */
int diga_bn_fwd_partials(const float* x, int64_t ld_x, float* y, int64_t ld_y, const float* residual, int64_t ld_r,
                         const float* gamma, const float* beta, float* running_mean, float* running_var,
                         float* save_mean, float* save_invstd, float* save_ab, int64_t M, int64_t C, int relu,
                         int y_twin, unsigned char* relu_bits, float momentum, float eps, const float* partial,
                         int64_t chunk_rows, void* workspace, size_t workspace_bytes, void* stream);

/* diga_bn_fwd_partials as the junction of a bottleneck whose skip branch ends in a BatchNorm of its own: `residual` is that branch's
 * RAW convolution output and residual_ab [2][C] its BatchNorm's coefficients (save_ab of a y = NULL call) --
 * y = relu(fma(x, a, b) + fma(residual, ar, br)), bit for bit what the two apply passes give, without the applied residual ever
 * being written.  ReLU always, fp32 y, no save_ab (a BatchNorm with residual keeps y or relu_bits for its backward). */
int diga_bn_fwd_partials_resab(const float* x, int64_t ld_x, float* y, int64_t ld_y, const float* residual, int64_t ld_r,
                               const float* residual_ab, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float* save_mean, float* save_invstd, int64_t M, int64_t C,
                               unsigned char* relu_bits, float momentum, float eps, const float* partial, int64_t chunk_rows,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ... replaced by RECORDS of unequal size: partial [n_records][3][C] {sum (x - s), sum (x - s)^2, s}, counts [n_records] = the rows
 * behind each record (0 allowed), sum of counts = M -- what the Winograd forward's output transform writes (stats_partial of
 * diga_conv2d_winograd_f32: its tile groups hold different numbers of in-image pixels).  workspace as diga_bn_fwd_partials + 96 floats. */
int diga_bn_fwd_records(const float* x, int64_t ld_x, float* y, int64_t ld_y, const float* residual, int64_t ld_r,
                        const float* gamma, const float* beta, float* running_mean, float* running_var,
                        float* save_mean, float* save_invstd, float* save_ab, int64_t M, int64_t C, int relu,
                        int y_twin, unsigned char* relu_bits, float momentum, float eps, const float* partial,
                        const float* counts, int64_t n_records, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the above wrt x (gamma/beta are frozen on this path): g = dy*mask, mask = [y>0] when y is given,
 * [fma(x, a, b) > 0] when relu_ab = save_ab of the forward is given instead (BN without residual), 1 when both are
 * null (no ReLU); dx = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)); dres (nullable) = g.  dx_twin != 0: dx (dense,
 * C % 8 == 0) receives the split twin instead of fp32 (the conv before this BN runs backward on the twin kernels). */
int diga_bn_bwd(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, const float* y, int64_t ld_y,
                const float* relu_ab, const float* gamma, const float* save_mean, const float* save_invstd, float* dx,
                int64_t ld_dx, float* dres, int64_t ld_dr, int64_t M, int64_t C, int training, int dx_twin, void* workspace,
                size_t workspace_bytes, void* stream);

/* diga_bn_bwd for a BatchNorm whose affine pair TRAINS -- the `linear_fuse` ConvModule of the SegFormer decode head,
 * G5/model/networks/segformer_head.py:63-68 (norm_cfg BN, requires_grad=True): additionally dgamma[c] = sum g*xhat and
 * dbeta[c] = sum g (in train mode the two column sums the input gradient needs anyway: no extra pass).  training = 0 (the module in
 * eval(): BN-frozen fine-tuning, test-time adaptation): save_mean / save_invstd are the RUNNING statistics the forward used,
 * dx = gamma*invstd*g without the mean terms, dgamma / dbeta as above -- what nn.BatchNorm2d returns in eval mode. */
int diga_bn_bwd_affine(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, const float* y, int64_t ld_y,
                       const float* relu_ab, const float* gamma, const float* save_mean, const float* save_invstd, float* dx,
                       int64_t ld_dx, float* dgamma, float* dbeta, int64_t M, int64_t C, int training, void* workspace,
                       size_t workspace_bytes, void* stream);

/* diga_bn_bwd for a gradient that arrives already masked and reduced: `g` and `partial` ([ceil(M/chunk_rows)][2][C]:
 * sum g, sum g*xhat per chunk) come out of the epilogue of the backward-data convolution that produced g
 * (diga_conv2d_nhwc_*_epi, chunk_rows = 128): one finalise launch + the apply pass (read g, x; write dx).
 * workspace >= 67*C floats. */
int diga_bn_bwd_partials(const float* g, int64_t ld_g, const float* x, int64_t ld_x, const float* gamma,
                         const float* save_mean, const float* save_invstd, float* dx, int64_t ld_dx, int64_t M, int64_t C,
                         int dx_twin, const float* partial, int64_t chunk_rows, void* workspace, size_t workspace_bytes,
                         void* stream);

/* GroupNorm over (HW x C/G) per image and group, then y = [relu](chan_scale[n,c] * (xhat*gamma + beta));
 * chan_scale (nullable, [N][C]) carries the Dropout2d keep/(1-p) pattern.  save_mean/invstd [N][G]. */
int diga_gn_fwd(const float* x, int64_t ld_x, float* y, int64_t ld_y, const float* gamma, const float* beta,
                const float* chan_scale, float* save_mean, float* save_invstd, int64_t N, int64_t HW, int64_t C,
                int64_t G, int relu, float eps, void* workspace, size_t workspace_bytes, void* stream);
int diga_gn_bwd(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, const float* y, int64_t ld_y,
                const float* gamma, const float* chan_scale, const float* save_mean, const float* save_invstd,
                float* dx, int64_t ld_dx, float* dgamma, float* dbeta, int64_t N, int64_t HW, int64_t C, int64_t G,
                void* workspace, size_t workspace_bytes, void* stream);

/* SE block pieces: out[n][c] = mean_hw x;  y = x*a[n][c] + b[n][c] (b nullable);  out[n][c] = sum_hw dy*x. */
int diga_avgpool_nhwc(const float* x, int64_t ld_x, float* out, int64_t N, int64_t HW, int64_t C, void* workspace,
                      size_t workspace_bytes, void* stream);
int diga_channel_affine(const float* x, int64_t ld_x, float* y, int64_t ld_y, const float* a, const float* b,
                        int64_t N, int64_t HW, int64_t C, void* stream);
/* The dense layers of the SE block (G5/model/seg_model_noaux.py:122-137: nn.Linear(1280, 80) -> ReLU -> nn.Linear(80, 1280) -> Sigmoid
 * on the pooled [N, 1280] vector; torch runs them through a GEMM library):  y[N][O] = act(x[N][K] . W[O][K]^T + b),
 * act 0 = none, 1 = ReLU, 2 = sigmoid.  Backward from the ACTIVATED output y: dz = dy * act'(y) (workspace dz [N][O], caller-owned),
 * db[O] = sum_n dz, dW[O][K] = dz^T x, dx[N][K] = dz W (db / dW / dx nullable). */
int diga_small_linear_fwd(const float* x, const float* w, const float* b, float* y, int64_t N, int64_t K, int64_t O, int act, void* stream);
int diga_small_linear_bwd(const float* x, const float* w, const float* y, const float* dy, float* dz, float* dx, float* dw, float* db,
                          int64_t N, int64_t K, int64_t O, int act, void* stream);
/* Bias gradient of a convolution with bias (the ASPP branches / bottleneck, G5/model/seg_model_noaux.py:143-170; torch computes
 * grad_output.sum((0, 2, 3))): out[c] = sum over the M rows of x [M][ld_x] (channels contiguous), shifted sums merged in double.
 * C % 4 == 0 and ld_x % 4 == 0, or any C <= 64 (the 19-class prediction conv of the SegFormer head, segformer_head.py:70).
 * workspace: diga_norm_workspace_bytes(M, 1, C). */
int diga_colsum_nhwc(const float* x, int64_t ld_x, float* out, int64_t M, int64_t C, void* workspace, size_t workspace_bytes,
                     void* stream);
int diga_channel_dot(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, float* out, int64_t N, int64_t HW,
                     int64_t C, void* workspace, size_t workspace_bytes, void* stream);

/* Multi-scale fusion of the SegFormer decode head (G5/model/networks/segformer_head.py:145-159: every embedded stage output is
 * resized to the 1/4-scale grid with F.interpolate(mode='bilinear', align_corners=False), :472-488, concatenated and reduced by the
 * 1x1 `linear_fuse` conv; resize and 1x1 conv commute, so the host applies the fuse weights at each map's own resolution and only the
 * SUM is formed at the fine scale): dst [N][H][W][C] (fp32, channels contiguous, C % 4 == 0, holds the finest map on entry)
 * += bias[c] (nullable) + sum_k resize(s_k [N][h_k][w_k][C]) for the non-null sources -- torch's half-pixel source index and tap order.
 * _bwd: the adjoint for ONE source, ds [N][h][w][C] = resize^T(dout) (the gradient wrt the finest map is dout itself); a gather
 * over each coarse pixel's footprint with the forward's weights, deterministic. */
int diga_pyramid_sum_fwd(float* dst, int64_t H, int64_t W, const float* bias, const float* s0, int64_t h0, int64_t w0,
                         const float* s1, int64_t h1, int64_t w1, const float* s2, int64_t h2, int64_t w2, int64_t N, int64_t C,
                         void* stream);
int diga_pyramid_sum_bwd(const float* dout, int64_t H, int64_t W, float* ds, int64_t h, int64_t w, int64_t N, int64_t C, void* stream);
/* The three adjoints of the SegFormer geometry in one pass over dout: ds2 [N][H/2][W/2][C], ds4 [N][H/4][W/4][C], ds8 [N][H/8][W/8][C]
 * (the stage maps of segformer_head.py:141-147 for a crop whose side is a multiple of 64); H % 16 == 0, W % 16 == 0, C % 16 == 0.
 * Same weights as diga_pyramid_sum_bwd, another summation order (fixed: deterministic). */
/* diga_pyramid_sum_fwd for that geometry (s2 / s4 / s8: the maps at 1/2, 1/4, 1/8 of dst's grid; H % 16 == 0, W % 16 == 0,
 * C % 32 == 0), tiled through LDS, the same taps in the same order; stats (nullable, [N * H * W / 64][3][C]) receives what the BatchNorm behind
 * `linear_fuse` needs -- per 64-pixel chunk and channel {sum (y - s), sum (y - s)^2, s}, the layout diga_bn_fwd_partials finalises
 * with chunk_rows = 64 (a chunk = four rows of a 16 x 16 tile; the finaliser only needs every chunk to hold 64 values). */
int diga_pyramid_sum_fwd3(float* dst, int64_t H, int64_t W, const float* bias, const float* s2, const float* s4, const float* s8,
                          float* stats, int64_t N, int64_t C, void* stream);
int diga_pyramid_sum_bwd3(const float* dout, int64_t H, int64_t W, float* ds2, float* ds4, float* ds8, int64_t N, int64_t C, void* stream);

/* One bilinearly resized map (align_corners=False, torch's half-pixel taps and tap order: the expressions of diga_pyramid_sum_fwd)
 * written into the C channels that start at dst of every pixel of a wider fine buffer: dst[n, y, x, 0:C] = resize(src)[n, y, x, :],
 * dst_ld floats between fine pixels (dst_ld >= C, % 4 == 0); nothing else of the buffer is written.  src [N,h,w,C] dense.  Upsampling
 * only (h <= H, w <= W; h == H and w == W is a plain copy: the bits, signed zeros, infinities and NaNs included), else DIGA_EINVAL.  diga_pyramid_resize_bwd is its exact adjoint on a
 * pitched fine gradient (dout_ld floats between fine pixels): a gather over every coarse pixel's footprint with the forward's weights
 * recomputed, no atomics, deterministic; ds [N,h,w,C] dense, every element written.  C % 4 == 0, pointers 16-byte aligned. */
int diga_pyramid_resize_fwd(const float* src, int64_t h, int64_t w, float* dst, int64_t dst_ld, int64_t H, int64_t W, int64_t N, int64_t C,
                            void* stream);
int diga_pyramid_resize_bwd(const float* dout, int64_t dout_ld, int64_t H, int64_t W, float* ds, int64_t h, int64_t w, int64_t N, int64_t C,
                            void* stream);

/* Depthwise 3x3 convolution, stride 1, padding = dilation, fp32 NHWC, pitched operands (csrc/dwconv.hip):
 *   y[n,i,j,c] = sum_{r,s} w9[3r+s][c] * x[n, i+(r-1)d, j+(s-1)d, c], zeros outside the map; w9 is [9][C], tap-major.
 * flip = 1 reads tap 8 - t in place of t: with x = dy that is the backward-data pass.  The nine products are added in tap order in one
 * fmaf chain from 0, a tap outside the map as an exact 0.  Every element of the C channels of every pixel of y is written (pass
 * uninitialised memory); columns C .. y_ld are not touched.  Exact fp32: no conv_math applies.
 * Rules (DIGA_EINVAL with a message, before any launch): non-null 16-byte aligned pointers; C % 4 == 0; x_ld, y_ld >= C, % 4 == 0 and
 * below 2^30; dilation >= 1; flip 0 or 1; x and y must not alias (two disjoint column windows of one matrix do not); extents below
 * 2^30 and N * H * W * ld of either operand at most 2^44.
 * N == 0: DIGA_OK without a launch.  Profiling tag: DIGA_PROF_ELEMENTWISE (work = 8 bytes per element). */
int diga_dwconv3x3_f32(const float* x, int64_t x_ld, const float* w9 /* [9][C], tap-major */, float* y, int64_t y_ld, int64_t N, int64_t H,
                       int64_t W, int64_t C, int64_t dilation, int flip, void* stream);
/* Its weight gradient: dw9[t][c] = sum over the pixels p of dy[p,c] * x[p + off_t, c].  Per-block partial sums go to the caller's
 * workspace (diga_dwconv3x3_wgrad_workspace_bytes; 0 for an unsupported shape), a second kernel adds them in block order: no float
 * atomics, bit-reproducible from run to run.  Rules as above, plus N > 0 and workspace_bytes >= the queried size. */
size_t diga_dwconv3x3_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C);
int diga_dwconv3x3_f32_wgrad(const float* dy, int64_t dy_ld, const float* x, int64_t x_ld, float* dw9 /* [9][C] */, void* workspace,
                             size_t workspace_bytes, int64_t N, int64_t H, int64_t W, int64_t C, int64_t dilation, void* stream);

/* 3x3 stride-2 pad-1 max-pool with ceil_mode (Ho = ceil((H-1)/2)+1 clipped so the last window starts inside);
 * idx [N,Ho,Wo,C] uint8 = winning tap (first maximum); backward gathers, no atomics. */
int diga_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int64_t N, int64_t H, int64_t W, int64_t C,
                          int64_t Ho, int64_t Wo, void* stream);
int diga_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int64_t N, int64_t H, int64_t W, int64_t C,
                          int64_t Ho, int64_t Wo, void* stream);

/* ------------------------------------------------------------------------------------
 * Colour-augmentation view: out = beta*Normalize(extra_aug(x)) + (1-beta)*x in one pass,
 * G5/train_DiGA_gta2city_warm_up.py:105-111,233 with extra_aug = kornia 0.5.8 ColorJitter -> RandomGrayscale ->
 * RandomGaussianBlur(3x3, sigma 2, reflect) -> RandomSharpness and Normalize = G5/util/utils.py:141-156.  kornia is not
 * part of the reference tree: PARITY UNPINNED against kornia, pinned against oracle/coloraug.py's restatement.
 * x, out [B,3,H,W] fp32 NCHW (device).  params [B][12] fp32 (device): {apply jitter, apply grayscale, apply blur,
 * apply sharpness} as 0/1, then brightness, contrast, saturation, hue factors, sharpness factor.  order (HOST int32[4]):
 * the permutation of {0 brightness, 1 contrast, 2 saturation, 3 hue} applied to every jittered sample.  mean, std:
 * HOST float[3].
 * ---------------------------------------------------------------------------------- */
int diga_color_aug_view(const float* x, float* out, const float* params, const int32_t* order_host, int64_t B, int64_t H,
                        int64_t W, float beta, const float* mean_host, const float* std_host, void* stream);

/* ------------------------------------------------------------------------------------
 * Object-contextual representations (csrc/ocr.hip): the two attention-shaped operations of the OCR head
 * (semi-supervised_segmentation/model/networks/ocrnet_module.py:24-44, 77-95, 231), K <= 32 "tokens" against a long pixel axis P.
 * Exact fp32 whatever the convolution arithmetic is; no floating-point atomics: sums over pixels are per-block partials (blocks of
 * 256 pixels) in `workspace`, added in block order by a second kernel -- two runs give the same bits.  No profiling tag.
 *
 * Common rules, all checked before anything touches a device (DIGA_EINVAL and a diga_last_error_string otherwise, a workspace
 * smaller than diga_ocr_workspace_bytes included): pointers non-null; tensors with a channel axis (x, dx, region, d_region, q,
 * dq, key, val, out, d_out, d_key, d_val, stat, workspace) 16-byte aligned, the K-wide ones (s, ds, attn) 4-byte aligned; pitches
 * (floats between consecutive pixels) >= the row and, on the channel tensors, % 4 == 0; 1 <= K <= 32; channel counts % 4 == 0 and
 * <= 1024; 1 <= N <= 65535; P >= 1.
 *
 * diga_ocr_workspace_bytes(N, P, K, C): C = the widest channel count of the call (region: C; attend_bwd: max(D, Dv)).  Monotone in
 *   every argument; 0 for a shape the entry points refuse.
 * diga_ocr_region_fwd: x [N][P][ld_x] (C used), s [N][P][ld_s] (K used) logits.  region [N][K][C] = sum_p softmax_p(s[n, :, k])[p]
 *   x[n, p, :], online: every block takes the maximum of its own 256 pixels, the reduce kernel rescales; accumulated, kept as partials
 *   and reduced in float64.  stat, N * K * (C + 2) floats for the backward pass: [N][K][C] what rounding the sum to fp32 `region`
 *   dropped (region + that = sum e x / sum e, normalised in float64, to ~2^-48), then [N][K][2] = (maximum, 1 / sum of exp(s - maximum)).  x and s are read once.
 * diga_ocr_region_bwd: with w = exp(s - max) / sum, g[p, k] = <d_region[k], x[p]>, dot[k] = <d_region[k], region[k]>:
 *   ds[p, k] = w (g - dot[k]), dx[p, :] = sum_k w[p, k] d_region[k, :] (written, not accumulated).  One pass over the pixels; dot and
 *   g - dot in float64 on region + its low-order part, so that sum_p ds[p, k] vanishes as far as a softmax backward's does.
 * diga_ocr_attend_fwd: q [N][P][ld_q] (D used), key [N][K][D], val [N][K][Dv] dense.  attn [N][P][K] = softmax_k(scale <q, key_k>)
 *   (nullable: not written), out [N][P][ld_out] (Dv used) = attn val.  (K * (D + Dv) + 64) * 4 bytes must fit the 160 KB of LDS.
 * diga_ocr_attend_bwd: dA = d_out val^T, dl = attn o (dA - sum_k attn dA); dq = scale dl key; d_key [N][K][D] = scale sum_p dl^T q,
 *   d_val [N][K][Dv] = sum_p attn^T d_out through the workspace partials (which also hold dl, [N][P][K]).
 * ---------------------------------------------------------------------------------- */
size_t diga_ocr_workspace_bytes(int64_t N, int64_t P, int64_t K, int64_t C);
int diga_ocr_region_fwd(const float* x, int64_t ld_x, const float* s, int64_t ld_s, float* region, float* stat, int64_t N, int64_t P,
                        int64_t K, int64_t C, void* workspace, size_t workspace_bytes, void* stream);
int diga_ocr_region_bwd(const float* x, int64_t ld_x, const float* s, int64_t ld_s, const float* stat, const float* region,
                        const float* d_region, float* dx, int64_t ld_dx, float* ds, int64_t ld_ds, int64_t N, int64_t P, int64_t K,
                        int64_t C, void* stream);
int diga_ocr_attend_fwd(const float* q, int64_t ld_q, const float* key, const float* val, float* out, int64_t ld_out, float* attn,
                        int64_t N, int64_t P, int64_t K, int64_t D, int64_t Dv, float scale, void* stream);
int diga_ocr_attend_bwd(const float* q, int64_t ld_q, const float* key, const float* val, const float* attn, const float* d_out,
                        int64_t ld_do, float* dq, int64_t ld_dq, float* d_key, float* d_val, int64_t N, int64_t P, int64_t K,
                        int64_t D, int64_t Dv, float scale, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Kernel-family timing (bench.py's roofline leg): when enabled, every entry point brackets its
 * launches with HIP events recorded on the launch stream.  Not for production steps.
 * ---------------------------------------------------------------------------------- */
enum {
    DIGA_PROF_CE2D = 0,
    DIGA_PROF_DISTILL,
    DIGA_PROF_UPSAMPLE_LOSS,
    DIGA_PROF_EMA,
    DIGA_PROF_SGD,
    DIGA_PROF_CLASSMIX_HIST,
    DIGA_PROF_CLASSMIX_PASTE,
    DIGA_PROF_CENTROID_WEIGHTS,
    DIGA_PROF_CONSENSUS,
    DIGA_PROF_CLASS_MEANS,
    DIGA_PROF_CENTROID_APPLY,
    DIGA_PROF_CONV_FWD,
    DIGA_PROF_CONV_BWD_DATA,
    DIGA_PROF_CONV_BWD_WEIGHT,
    DIGA_PROF_NORM,
    DIGA_PROF_ELEMENTWISE,
    DIGA_PROF_MIT_GEMM,        /* fp16 Linear / patch-embedding GEMMs, forward and backward-data (include/diga_mit.h) */
    DIGA_PROF_MIT_WGRAD,       /* fp16 weight-gradient GEMMs */
    DIGA_PROF_MIT_ATTN_FWD,    /* spatial-reduction attention, forward */
    DIGA_PROF_MIT_ATTN_BWD,    /* spatial-reduction attention, backward (dQ, dK/dV) */
    DIGA_PROF_MIT_NORM,        /* LayerNorm forward / backward */
    DIGA_PROF_MIT_DWCONV,      /* depthwise 3x3 + GELU (Mix-FFN), forward / backward */
    DIGA_PROF_MIT_MISC,        /* im2col / col2im, casts, column sums */
    DIGA_PROF_NTAGS
};
int diga_prof_enable(int on);
int diga_prof_reset(void);
/* Waits for the recorded events of `tag`; h_count = launches seen, h_total_ms = summed duration. */
int diga_prof_query(int tag, int64_t* h_count, double* h_total_ms);
/* Summed ALGORITHMIC work the recorded calls of `tag` declared: bytes (HBM-bound families: what the call must move
 * given its arguments, e.g. 8 B per element for a BatchNorm apply, +4 with a residual) or FLOPs (convolutions:
 * 2*M*Cout*R*S*Cin). */
int diga_prof_query_work(int tag, double* h_work);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DIGA_HIP_H */
