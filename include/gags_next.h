/*
 * gags_next.h -- C ABI of the kernels either side of the rasterizer (N5), same
 * library (libgags_hip.so) and conventions as gags_raster.h: extern "C", device pointers, caller-owned memory,
 * `stream` = hipStream_t as void*, return GAGS_OK or a negative GAGS_E* code.  fp32 unless noted.
 *
 * Feature / scale maps are CHANNEL-MAJOR [C, H, W] as everywhere in the reference after
 * gaussian_renderer/__init__.py:73 (`permute(2, 0, 1)`); a segmentation map holds segment ids as floats, -1 = none
 * (scene/cameras.py seg_map, preprocess.py:332-336).
 */
#ifndef GAGS_NEXT_H
#define GAGS_NEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only what these headers declare is exported */
#pragma GCC visibility push(default)

/* ---- N2: losses and ground-truth assembly of train.py:149-172 -------------------------------------------------- */

/* utils/loss_utils.py:138-154 get_trained_seg: 5x5 mean filter (zero padded) of scale_map[3,h,w], arg-max level,
 * out[h,w] = seg_map[1 + level] (seg_map[4,h,w]).  No gradient (arg-max). */
int gags_trained_seg(int h, int w, const float *seg_map, const float *scale_map, float *out, void *stream);

/* utils/loss_utils.py:59-66 scale_regulation_loss: acc[0] += sum(-s * log(s + 1e-6)) over n values (acc: one
 * double, zeroed by the caller; loss = acc / n).  Backward: v_s[i] = -(log(s + eps) + s / (s + eps)) * v_over_n. */
int gags_entropy_fwd(int64_t n, const float *s, double *acc, void *stream);
int gags_entropy_bwd(int64_t n, const float *s, float v_over_n, float *v_s, void *stream);
/* the same with the cotangent v[0] read on the device (v_over_n = v[0] / n): no host readback inside a backward pass */
int gags_entropy_bwd_dev(int64_t n, const float *s, const float *v, float *v_s, void *stream);

/* Per-segment first and second moments of a channel-major map x[c, n_pix] under the segment map seg[n_pix]
 * (ids in [0, n_seg), anything negative = no segment): s1[n_seg, c], s2[n_seg, c] (double) and cnt[n_seg], all
 * zeroed by the caller.  This is the one pass over the pixels behind both segment losses, which the reference
 * computes with a Python loop over the segment ids (utils/loss_utils.py:47-54 Scale_balance_loss with c = 1,
 * :117-133 scale_region_regulation_loss with c = the feature width). */
int gags_segment_stats(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, double *s1, double *s2,
                       int32_t *cnt, void *stream);
/* The same with `copies` private accumulator sets s1 / s2 [copies, n_seg, c], cnt [copies, n_seg] (zero-filled by the
 * caller, summed by the caller): a workgroup adds into set (block index mod copies).  The double atomics serialize per
 * address at the memory side; with a few hundred segments per image that, not bandwidth, bounds the one-set kernel.
 * layout 1: x is pixel-major [n_pix, c] (the rasterizer's own memory under the [C,H,W] view: no `.contiguous()` copy). */
int gags_segment_stats_multi(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, int copies, double *s1,
                             double *s2, int32_t *cnt, int layout, void *stream);
/* The same moments by runs of equal ids (round 6; csrc/seg_losses.hip segment_stats_runs_kernel): no atomics in global memory, the
 * cost per pixel independent of how finely the map is cut.  Serves c == 16 pixel-major (layout 1) and c == 1 with
 * n_seg * (16 c + 4) <= 150 KB; gags_segment_stats_runs_copies returns the number of private copies s1 / s2 / cnt must hold
 * ([copies, n_seg, c], [copies, n_seg]; every element is written: no zero fill), or 0 when the shape is not served -- use
 * gags_segment_stats_multi then.  The caller sums the copies. */
int gags_segment_stats_runs_copies(int64_t n_pix, int c, int n_seg, int layout);
int gags_segment_stats_runs(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, int copies, double *s1,
                            double *s2, int32_t *cnt, int layout, void *stream);
/* The two segment losses from the moments' private copies ([copies, n_seg, c] doubles, [copies, n_seg] counts, as left by
 * gags_segment_stats_multi / _runs), in two launches: the copies summed in copy order into s1 / s2 [n_seg, c] and cnt [n_seg], then
 *   mode 0 (c == 1), Scale_balance_loss (utils/loss_utils.py:32-57, mix_seg=True): loss[0] = mean over the present segments of
 *           the segment's mean; coef[i] = 1 / (n_i K), 0 for an absent segment (K = present segments, at least 1);
 *   mode 1, scale_region_regulation_loss (:103-136, mix_seg=True): loss[0] = sum over segments of >= 2 pixels of
 *           n_i mean_c var_c / n_pix (unbiased variance, clamped at 0); mean[n_seg, c] and coef[i] = 2 n_i / ((n_i - 1) c n_pix).
 * All arithmetic in double, results rounded to float once. */
int gags_segment_loss(int mode, int n_seg, int c, int copies, int64_t n_pix, const double *s1c, const double *s2c,
                      const int32_t *cntc, double *s1, double *s2, int32_t *cnt, float *loss, float *coef, float *mean,
                      void *stream);
/* Backward of the region-variance loss: v_x[c, p] = coef[seg(p)] * (x[c, p] - mean[seg(p), c]), 0 outside segments. */
int gags_region_var_bwd(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, const float *mean,
                        const float *coef, float *v_x, void *stream);
/* ... with x and v_x pixel-major [n_pix, c] when layout = 1. */
int gags_region_var_bwd_layout(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, const float *mean,
                               const float *coef, float *v_x, int layout, void *stream);
/* The same for a pixel-major map (c % 4 == 0, 16-byte aligned) with another consumer's gradient of that map added on the way
 * out: v_x = add + coef[seg] (x - mean[seg]) -- one pass instead of this kernel's and an element-wise sum's. */
int gags_region_var_bwd_add(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, const float *mean,
                            const float *coef, const float *add, float *v_x, void *stream);
/* Backward of the segment-balanced mean: out[p] = coef[seg(p)], 0 outside segments. */
int gags_gather_seg_coef(int64_t n_pix, const float *seg, int n_seg, const float *coef, float *out, void *stream);

/* scene/dataset_readers.py:54-121 read_sam_clip_feature (default mode): for the three granularity levels l = 1..3 of
 * seg_map[4, h, w] gather img_embed[n_emb, c] rows (id -1 reads the LAST row, as Python indexing does), resize
 * bilinearly (align_corners) to the scale map's [H, W] and blend with scale_map[3, H, W]:
 *     feature_map[c, H, W] = sum_l F_l * scale_map[l],   mask[H, W] = all three ids != -1 (nearest resize), 0/1.
 * _bwd_scale: v_scale[l, H, W] = sum_c v_feature[c] * F_l[c]  (scale_map comes from the trainable scale decoder). */
int gags_sam_clip_feature(int c, int H, int W, int h, int w, int n_emb, const float *img_embed, const float *seg_map,
                          const float *scale_map, float *feature_map, float *mask, void *stream);
int gags_sam_clip_feature_bwd_scale(int c, int H, int W, int h, int w, int n_emb, const float *img_embed,
                                    const float *seg_map, const float *v_feature, float *v_scale, void *stream);
/* The same function with max_mode=True (:81-88; what render.py:64,154 asks for), forward only: k = argmax_l scale_map[l]
 * (the lowest index among equal maxima), one_hot = its indicator, valid_l = (level l's id at the nearest-resized source pixel
 * != -1):  feature_map = (F_s one_hot[0]) valid_s + (F_m one_hot[1]) valid_m + (F_l one_hot[2]) valid_l  in the reference's
 * order -- F_k where level k is valid, else 0 -- and mask[H, W] = feature_map[0] != 0 (channel 0 ALONE, as the reference), 0/1. */
int gags_sam_clip_feature_max(int c, int H, int W, int h, int w, int n_emb, const float *img_embed, const float *seg_map,
                              const float *scale_map, float *feature_map, float *mask, void *stream);

/* train.py:165-166 fused: l1_map[H, W] = mean_c |pred * mask - gt * mask| with gt, mask = read_sam_clip_feature(...)
 * WITHOUT materialising the [c, H, W] ground truth (4.25 GB at 1080p x 512) or the two masked copies.
 * Backward for a cotangent v_map[H, W]: v_pred[c, H, W] and v_scale[3, H, W]. */
/* layout: 0 = pred (and v_pred) are [c, H, W]; 1 = they are [H, W, c] (the memory behind the decoder's output when
 * gags_decoder_head wrote it pixel-major): nothing is transposed, every access is a row. */
int gags_distill_l1_map_fwd(int c, int H, int W, int h, int w, int n_emb, const float *pred, const float *img_embed,
                            const float *seg_map, const float *scale_map, float *l1_map, float *mask, int layout,
                            void *stream);
int gags_distill_l1_map_bwd(int c, int H, int W, int h, int w, int n_emb, const float *pred, const float *img_embed,
                            const float *seg_map, const float *scale_map, const float *v_map, float *v_pred,
                            float *v_scale, int layout, void *stream);

/* CNN_decoder's normalising head fused with the distillation L1 (train.py:159-166): from the last layer's fp32 logits
 * x[H*W, ld] (c = ld = 512: the reference's CNN_decoder(16, 512); other widths: GAGS_EINVAL, use the two entries) to
 *     l1_map[H, W] = mean_c | normalize(x) * mask - gt * mask |,   gt, mask = read_sam_clip_feature(...)
 * and back: d l1_map -> dz[H*W, ld] bf16 (gradient of the logits; what gags_decoder_head_bwd would have produced from
 * the loss's [c,H,W] gradient) and v_scale[3, H, W].  The normalised [c,H,W] map and its gradient never exist. */
int gags_decoder_head_distill_fwd(int c, int ld, int H, int W, int h, int w, int n_emb, const float *x,
                                  const float *img_embed, const float *seg_map, const float *scale_map,
                                  float *l1_map, float *mask, void *stream);
int gags_decoder_head_distill_bwd(int c, int ld, int H, int W, int h, int w, int n_emb, const float *x,
                                  const float *img_embed, const float *seg_map, const float *scale_map,
                                  const float *v_map, void *dz_bf16, float *v_scale, void *stream);
/* ... with the logits' gradient in fp32 (dz[H*W, ld] float): the fp32-tensor decoder tiers ("exact", "bf16x2"). */
int gags_decoder_head_distill_bwd_f32(int c, int ld, int H, int W, int h, int w, int n_emb, const float *x,
                                      const float *img_embed, const float *seg_map, const float *scale_map,
                                      const float *v_map, float *dz, float *v_scale, void *stream);

/* ---- N1: the per-pixel decoders (models/networks.py:109-248: stacks of 1x1 convolutions) ---------------------- */

/* fp32 pixel-major x[n_pix, c] (the rasterizer's own [H, W, D] output) -> bf16 y[n_pix, c_pad], zero-padded
 * (c_pad % 32 == 0). */
int gags_decoder_pack_input(int64_t n_pix, int c, int c_pad, const float *x, void *y_bf16, void *stream);
/* One 1x1-conv layer's parameters (w [co, ci] fp32 = Conv2d.weight[:, :, 0, 0], b [co]) in every form the bf16 kernels read,
 * dimensions zero-padded to multiples of 32 (Np, Kp): w_bf16 [Np, Kp] and its transpose wt_bf16 [Kp, Np] row-major, both
 * again in MFMA-fragment order ([R / 32][C / 16][2][32][8]: the A operand of one v_mfma_f32_32x32x16_bf16 as one
 * contiguous kilobyte) for the fused kernels, and the padded fp32 bias.  Round-to-nearest-even, as torch's cast. */
int gags_decoder_pack_layer(int co, int ci, const float *w, const float *b, void *w_bf16, void *wt_bf16, void *w_frag,
                            void *wt_frag, float *bias_pad, void *stream);
/* Every layer of a decoder in one launch: the arguments of gags_decoder_pack_layer as arrays of n_layers (<= 12) entries. */
int gags_decoder_pack_layers(int n_layers, const int *co, const int *ci, const float *const *w, const float *const *b,
                             void *const *w_bf16, void *const *wt_bf16, void *const *w_frag, void *const *wt_frag,
                             float *const *bias_pad, void *stream);

/* One 1x1-convolution layer as a GEMM on the 16-bit matrix cores (bf16 operands, fp32 accumulate):
 *     y[p, n] = act( sum_k (a1[p, k] + a2[p, k]) * w[n, k] + bias[n] ) * (mask_src[p, n] > 0) + residual[p, n]
 * a1, a2 (optional: the residual sums x1 + x2 / x3 + x4 of CNN_decoder.forward), w, mask_src (optional), residual
 * (optional), y_bf16: bf16; bias (optional), y_f32 (optional second output): fp32.  k_in % 32 == 0, n_out % 8 == 0.
 * The backward's input-gradient GEMM is the same call with w = W^T, mask_src = the layer below's output (its ReLU
 * mask) and residual = the gradient arriving over a skip connection. */
int gags_decoder_layer(int64_t n_pix, int n_out, int k_in, const void *a1, const void *a2, const void *w,
                       const float *bias, int relu, const void *mask_src, const void *residual, void *y_bf16,
                       void *y_premask_bf16, float *y_f32, void *stream);
/* (y_premask_bf16, optional: the value before the mask -- the gradient that also travels over a skip connection.) */

/* Weight and bias gradient of one layer: d_w[n_out, k_in] = sum_p dz[p, n] * (a1[p, k] + a2[p, k]),
 * d_b[n_out] = sum_p dz[p, n] (d_b optional); both fp32, OVERWRITTEN.  No atomics: every pixel chunk leaves a partial
 * matrix in `scratch` (gags_decoder_wgrad_scratch_bytes) and the partials are summed in chunk order -- bit-reproducible.
 * dz, a1, a2 (optional): bf16 pixel-major.  n_out % 16 == 0, k_in % 16 == 0. */
int64_t gags_decoder_wgrad_scratch_bytes(int64_t n_pix, int n_out, int k_in);
int gags_decoder_wgrad(int64_t n_pix, int n_out, int k_in, const void *dz, const void *a1, const void *a2, float *d_w,
                       float *d_b, void *scratch, int64_t scratch_bytes, void *stream);
/* The same gradient written in the parameter's own shape (round 6): d_w[co, ci] and d_b[co] are the leading co x ci block of the
 * padded [n_out, k_in] product (co <= n_out, ci <= k_in: what nn.Conv2d(ci, co, 1).weight.grad holds, models/networks.py:145-149),
 * every sum multiplied by out_scale[0] when given (a device scalar: the f16 tier's power of two) -- no slice copy and no
 * element-wise multiply per parameter after the call.  Same sums, same order, same bits as gags_decoder_wgrad. */
int gags_decoder_wgrad_out(int64_t n_pix, int n_out, int k_in, const void *dz, const void *a1, const void *a2, float *d_w,
                           float *d_b, int co, int ci, const float *out_scale, void *scratch, int64_t scratch_bytes,
                           void *stream);

/* Backward of gags_decoder_head: cotangent g (layout 0: [c, n_pix], 1: [n_pix, c]) + the saved logits x[n_pix, ld] ->
 * pixel-major bf16 dz[n_pix, ld]. */
int gags_decoder_head_bwd(int64_t n_pix, int c, int ld, int mode, const float *x, const float *g, void *dz_bf16,
                          int layout, void *stream);

/* bf16 x[n_pix, ld] -> fp32 y[n_pix, c] (first c columns): the decoder's input gradient in the rasterizer's own
 * [H, W, D] layout. */
int gags_decoder_unpack_grad(int64_t n_pix, int c, int ld, const void *x_bf16, float *y, void *stream);

/* Output head: pixel-major fp32 logits x[n_pix, ld] (first c columns) -> out; mode 0 = F.normalize(dim=0)
 * (CNN_decoder, :192), mode 1 = softmax over channels (CNN_scale_decoder, :242).
 * layout 0: CHANNEL-major out[c, n_pix] (the reference's contiguous [C, H, W]); layout 1 (c % 4 == 0, ld <= 512,
 * ld % 32 == 0): PIXEL-major out[n_pix, c] -- the caller views it as [C, H, W] through a permute, exactly like the
 * rasterizer's output, and nothing is transposed on the way in or out. */
int gags_decoder_head(int64_t n_pix, int c, int ld, int mode, const float *x, float *out, int layout, void *stream);

/* CNN_decoder's whole forward chain (models/networks.py:172-190: nine 1x1 convolutions, x3 = conv(x1 + x2),
 * x5 = conv(x3 + x4)) in ONE kernel, bf16 mode: 64-pixel tiles, activations resident in LDS, weights streamed from L2.
 * x [n_pix, c_in] fp32 (c_in <= 32); w_bf16[9]: the padded bf16 matrices gags_decoder_layer takes ([256, 32], 7 x [256,
 * 256], [n_last, 256]) re-ordered into MFMA fragments: [N / 32][K / 16][lane = 32 kh + n][8 values k = 16 s + 8 kh ..]; bias[9] fp32; acts_bf16[9] (or NULL, or NULL entries): a0 [n_pix, 32] and the eight hidden
 * activations [n_pix, 256] kept for the backward -- entries 3 and 6 hold the residual SUMS x1 + x2 and x3 + x4 (the inputs
 * of layers 3 and 6: what their weight gradients contract), not x2 / x4 --; logits [n_pix, n_last] fp32, n_last % 256 == 0.
 * Bit-identical to the same chain run through gags_decoder_layer. */
int gags_decoder_fwd_fused(int64_t n_pix, int c_in, int n_last, const float *x, const void *const *w_bf16,
                           const float *const *bias, void *const *acts_bf16, void *masks, float *logits, void *stream);
/* (masks, optional: uint32 [8, n_pix rounded up to a multiple of 64, 8] -- the ReLU decisions [activation > 0] of the eight hidden activations as bits, word
 * n / 32 of a pixel for channel n; the bit order inside a word is private to this kernel and gags_decoder_bwd_fused, which
 * reads the words instead of the activations themselves: an opaque buffer to the caller.) */

/* ... and the nine input-gradient GEMMs of its backward in one kernel: dz_last [n_pix, n_last] bf16 (from the head's
 * backward) -> dz_bf16[0..7] = the gradients at the outputs of layers 0..7 ([n_pix, 256] bf16 each, what the weight
 * gradients contract), gin [n_pix, c_in] fp32 (optional).  wt_bf16[9]: the TRANSPOSED padded matrices ([32, 256], 7 x
 * [256, 256], [256, n_last]) in the same fragment order; masks: the bit masks gags_decoder_fwd_fused kept (the two skip gradients stay in registers).  Bit-identical to the chain of gags_decoder_layer calls with mask_src / residual / y_premask. */
int gags_decoder_bwd_fused(int64_t n_pix, int c_in, int n_last, const void *dz_last_bf16, const void *const *wt_bf16,
                           const void *masks, void *const *dz_bf16, float *gin, void *stream);
/* (the same with the input gradient multiplied by the device scalar gin_scale[0] on its way out -- the f16 tier's 1 / S) */
int gags_decoder_bwd_fused_scaled(int64_t n_pix, int c_in, int n_last, const void *dz_last_bf16, const void *const *wt_bf16,
                                  const void *masks, void *const *dz_bf16, float *gin, const float *gin_scale, void *stream);

/* CNN_scale_decoder (models/networks.py:220-248: 16 -> 64 -> 128 -> 64 -> 32 -> 16 -> 3) as one kernel, bf16 mode: x
 * [n_pix, c_in <= 32] fp32; w_bf16[6]: the padded matrices [64,32] [128,64] [64,128] [32,64] [32,32] [32,32] in MFMA-
 * fragment order ([N / 32][K / 16][64][8]); bias[6] fp32 [N_pad]; acts_bf16[6] (optional): a0 [n_pix, 32] and the five
 * hidden activations [n_pix, 64 / 128 / 64 / 32 / 32] kept for the weight gradients; masks (optional): uint32 [n_pix, 11],
 * the ReLU decisions of the five hidden activations as bits (words 0-1, 2-5, 6-7, 8, 9 + one spare); logits [n_pix, 32]
 * fp32 (3 real columns).  Bit-identical to the same chain run through gags_decoder_layer. */
int gags_scale_decoder_fwd_fused(int64_t n_pix, int c_in, const float *x, const void *const *w_bf16,
                                 const float *const *bias, void *const *acts_bf16, void *masks, float *logits, void *stream);
/* The same with the decoder's head fused in (round 6): softmax3 [3, n_pix] fp32 channel-major = softmax over the three real
 * logits (CNN_scale_decoder.forward's last line, models/networks.py:248), bit-identical to gags_decoder_head(mode 1) on the
 * logits; `logits` may then be NULL (nothing needs them: gags_softmax_head_bwd_y works from the output). */
int gags_scale_decoder_fwd_fused_head(int64_t n_pix, int c_in, const float *x, const void *const *w_bf16,
                                      const float *const *bias, void *const *acts_bf16, void *masks, float *logits,
                                      float *softmax3, void *stream);
/* Backward of a softmax head of c <= 4 channels from its output: y, g [c, n_pix] fp32 -> dz [n_pix, ld] 16-bit (columns >= c
 * zero), dz = y (g - <y, g>): what gags_decoder_head_bwd(mode 1, layout 0) computes from the logits, bit for bit. */
int gags_softmax_head_bwd_y(int64_t n_pix, int c, int ld, const float *y, const float *g, void *dz_bf16, void *stream);

/* ... and the five input-gradient GEMMs of its backward in one kernel: dz_last [n_pix, 32] bf16 (from the head's backward)
 * -> dz_bf16[0..4] = the gradients at the outputs of layers 0..4 ([n_pix, 64 / 128 / 64 / 32 / 32] bf16: what the weight
 * gradients contract).  wt_bf16[1..5]: the TRANSPOSED padded matrices ([64,128]... = W_i^T [K_i, N_i]) in fragment order
 * (entry 0 unused); masks: what gags_scale_decoder_fwd_fused kept.  Bit-identical to the chain of gags_decoder_layer calls
 * with mask_src. */
int gags_scale_decoder_bwd_fused(int64_t n_pix, const void *dz_last_bf16, const void *const *wt_bf16, const void *masks,
                                 void *const *dz_bf16, void *stream);

/* ---- N1 at the reference's precision (models/networks.py:109-248 are fp32 Conv2d stacks) ------------------------- */

/* The same layer as gags_decoder_layer with fp32 tensors and fp32-equivalent arithmetic: every operand enters the 16-bit
 * matrix cores as three bfloat16 terms (h + m + l = the fp32 value, exactly) and a product as its six terms of order
 * <= 2 (dropped: <= 2^-24 relative), fp32 accumulation.  a1, a2 (optional), mask_src, residual, y, y_premask: fp32 with
 * leading dimensions lda (inputs) / ldy (everything [n_pix, n_out]-shaped); w [n_out, k_in]; any n_out, k_in >= 1. */
int gags_decoder_layer_exact(int64_t n_pix, int n_out, int k_in, const float *a1, const float *a2, int lda, const float *w,
                             const float *bias, int relu, const float *mask_src, const float *residual, float *y,
                             float *y_premask, int ldy, void *stream);

/* The same two kernels with the number of bfloat16 terms per operand as an argument.  terms = 3: the calls above.
 * terms = 2 (the "bf16x2" tier of gags_amd/decoders.py): h + m = 16 significand bits per operand, three matrix terms per
 * product (h h' + h m' + m h'), relative error <= ~2^-16 per product -- the reference's nn.Conv2d stacks
 * (models/networks.py:145-149, 229-233) run in TF32 (10-bit significands) under torch's defaults on the GPU its README
 * names (README.md:26-31), so this tier is still 32x tighter than the reference's own arithmetic, at half the matrix work. */
int gags_decoder_layer_split(int64_t n_pix, int n_out, int k_in, const float *a1, const float *a2, int lda, const float *w,
                             const float *bias, int relu, const float *mask_src, const float *residual, float *y,
                             float *y_premask, int ldy, int terms, void *stream);
int gags_decoder_wgrad_split(int64_t n_pix, int n_out, int k_in, const float *dz, int lddz, const float *a1,
                             const float *a2, int lda, float *d_w, float *d_b, void *scratch, int64_t scratch_bytes,
                             int terms, void *stream);

/* Weight and bias gradient at the same precision, WITHOUT atomics: pixel chunks -> partial matrices in `scratch` ->
 * summed in chunk order (bit-reproducible).  d_w [n_out, k_in] and d_b [n_out] (optional) are overwritten. */
int64_t gags_decoder_wgrad_exact_scratch_bytes(int64_t n_pix, int n_out, int k_in);
int gags_decoder_wgrad_exact(int64_t n_pix, int n_out, int k_in, const float *dz, int lddz, const float *a1,
                             const float *a2, int lda, float *d_w, float *d_b, void *scratch, int64_t scratch_bytes,
                             void *stream);

/* Backward of the output heads with an fp32 result dz[n_pix, lddz] (columns >= c zero); x = the logits [n_pix, ldx];
 * g: layout 0 = [c, n_pix], 1 = [n_pix, c]; modes as gags_decoder_head. */
int gags_decoder_head_bwd_exact(int64_t n_pix, int c, int ldx, int mode, const float *x, const float *g, int layout,
                                float *dz, int lddz, void *stream);

/* ---- N4: query-time relevancy (eval/openclip_encoder.py:42-56, 96-111) ---------------------------------------- */

/* For every pixel embedding embed[n_pix, c] and every positive phrase j: the LERF relevancy pair
 * probs[j, n_pix, 2] = softmax(10 * (sim_pos_j, sim_neg_k*)) with k* the negative phrase that minimises the positive
 * probability.  pos[n_pos, c], neg[n_neg, c] are unit text embeddings.  One read of the embeddings for all phrases. */
int gags_relevancy(int64_t n_pix, int c, int n_pos, int n_neg, const float *embed, const float *pos, const float *neg,
                   float *probs, void *stream);

/* The rest of the query path of one view (evaluate_iou_loc.py:100-146 `activate_stream`, :163-176
 * `lerf_localization`), for all phrases at once and without leaving the GPU.  valid_map[n_phrases, h, w] = the
 * relevancy maps get_max_across returned (one level).  Per phrase:
 *   avg      = 30x30 box mean of valid_map (cv2.filter2D with ones/900: anchor box/2, BORDER_REFLECT_101)   (:108-111)
 *   blended  = 0.5 * (avg + valid_map)                                      the heat map                      (:113)
 *   output   = clip(((blended - min) / (max - min + 1e-9)) * 2 - 1, 0, 1)                                     (:131-135)
 *   mask_pred   = output > thresh                                            uint8                             (:137)
 *   mask_smooth = eval/utils.py:55-64 smooth(mask_pred): (2 s + 1)^2 majority with the reference's own window bounds (:138)
 *   stats[k] = {min(blended), max(blended), max(avg)}; max(avg) is lerf_localization's score (:174), its position(s)
 *              are where avg == stats[k][2].
 * scratch: gags_relevancy_activate_scratch_bytes() bytes. */
int64_t gags_relevancy_activate_scratch_bytes(int n_phrases, int h, int w);
int gags_relevancy_activate(int n_phrases, int h, int w, const float *valid_map, float thresh, int box, int smooth_scale,
                            float *avg, float *blended, float *output, unsigned char *mask_pred,
                            unsigned char *mask_smooth, float *stats, void *scratch, int64_t scratch_bytes, void *stream);

/* ---- N5: 3-D open-vocabulary query on the Gaussians (compute_relvancy.py:273-394 `pcd_relvancy`, --pcd_mode) ------- */

/* compute_relvancy.py:363-367 for every phrase k of probs[n_phrases, n, 2] (gags_relevancy's output over the n Gaussians;
 * column 0 is the relevancy r), in the reference's fp32 order:
 *   normalized[k, i] = clip(((r_i - min r) / ((max r - min r) + 1e-9)) * 2 - 1, 0, 1)
 *   mask[k, i]       = normalized[k, i] > rel_thresh                          uint8
 * min / max stay on the device.  n == 0 or n_phrases == 0: nothing to do.  scratch: the _scratch_bytes() bytes. */
int64_t gags_point_relevancy_mask_scratch_bytes(int n_phrases, int64_t n);
int gags_point_relevancy_mask(int n_phrases, int64_t n, const float *probs, float rel_thresh, float *normalized,
                              unsigned char *mask, void *scratch, int64_t scratch_bytes, void *stream);

/* utils/pcd_utils.py:204-219 smooth_pcd_mask for n_masks masks mask[n_masks, n] (uint8, nonzero = set) over the points
 * xyz[n, 3] at once.  For every mask k and point i:
 *   c = #{ j : mask[k, j] and ((dx*dx + dy*dy) + dz*dz) <= radius*radius }   in IEEE float64 from the float32
 *       coordinates, no FMA (the point itself included: scipy's KDTree.query_ball_point rule)
 *   out[k, i] = c > threshold || (mask[k, i] && c >= 10)                      (10 is the reference's own constant)
 * counts[k, i] = min(c, max(threshold + 1, 10)) when counts is not NULL (no count is needed past that).  No atomics on the
 * results: bit-reproducible.  Requires n_masks * n < 2^31, n_masks <= 65534, radius finite and > 0, threshold >= 0.
 * scratch: the _scratch_bytes() bytes (0 when nothing runs). */
int64_t gags_point_mask_smooth_scratch_bytes(int n_masks, int64_t n);
int gags_point_mask_smooth(int n_masks, int64_t n, const float *xyz, const unsigned char *mask, double radius, int threshold,
                           unsigned char *out, int32_t *counts, void *scratch, int64_t scratch_bytes, void *stream);


/* ---- N6: depth_SAM.py, the point-to-pixel min-depth mapping of the GAS stage ---------------------------------------------
 * n points xyz[n, 3], n_cams cameras: viewmats[C, 4, 4] row-major world-to-camera (world_view_transform.T), Ks[C, 3, 3]
 * ([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), rendered depths[C, h, w] (channel 3 of render(..., render_mode="RGB+ED")).  For
 * point i and camera c, all fp32, no FMA, IEEE division (depth_SAM.py:34-77 compute_mapping):
 *   1. (xc, yc, zc) = rows 0..2 of M (x, y, z, 1) as ((M[r,0] x + M[r,1] y) + M[r,2] z) + M[r,3]
 *   2. u = (xc fx) / zc + cx,  v = (yc fy) / zc + cy
 *   3. ui = rint(u), vi = rint(v), half to even (torch.round)
 *   4. inside <=> cut_bound <= ui < w - cut_bound and cut_bound <= vi < h - cut_bound, compared in float (NaN, +-inf and
 *      anything past the int32 range are outside)
 *   5. d = depths[c, vi, ui]; visible <=> inside and |d - zc| <= vis_thresh d
 * mapping[i, c] = (vi, ui), visible[i, c] = 1 when visible, else (0, 0) and 0;  min_depth[i] = min over the cameras that see
 * i of d (+inf when none);  samples[c, v, u] = min_depth[j] for the HIGHEST index j visible in c at (v, u), else 0.
 * Requires n < 2^31 - 1, n_cams >= 1, 1 <= h, w < 2^24, h w < 2^31, cut_bound >= 0; offsets into the outputs are 64-bit.  Bit-
 * reproducible (the scatter's only atomic is an integer max of the point index).  scratch: the _scratch_bytes() bytes,
 * 0 when n == 0. */
int64_t gags_depthsample_scratch_bytes(int64_t n, int n_cams, int h, int w);
/* min_depth[n]; mapping[n, n_cams, 2] int32 and visible[n, n_cams] uint8 are optional (NULL: not written) */
int gags_depthsample_map(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats, const float *Ks,
                         const float *depths, float vis_thresh, int cut_bound, float *min_depth, int32_t *mapping,
                         unsigned char *visible, void *scratch, int64_t scratch_bytes, void *stream);
/* samples[n_cams, h, w] from min_depth[n] (gags_depthsample_map's, same arguments); n == 0: all zero */
int gags_depthsample_scatter(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats, const float *Ks,
                             const float *depths, float vis_thresh, int cut_bound, const float *min_depth, float *samples,
                             void *scratch, int64_t scratch_bytes, void *stream);

/* N22: the same mapping for a rig of any cameras the rasterizer renders (gags_raster.h: GAGS_CAM_PINHOLE / _ORTHO / _FISHEYE,
 * the fisheye's distortion coefficients k1 .. k4 of GAGS_PROJ_KB), models mixed freely.  Steps 1 and 3-5 above hold for every
 * model; only step 2 depends on the camera's model, all fp32, no FMA, IEEE division:
 *   pinhole   step 2 above, verbatim.  No cull.
 *   ortho     u = xc fx + cx,  v = yc fy + cy
 *   fisheye   the quantities of the projection (gags_raster.h "GAGS_CAM_FISHEYE", "GAGS_PROJ_KB"), eps = 1e-7:
 *               rho = sqrt(xc xc + yc yc) + eps,  theta = atan2f(rho, zc + eps),  t = theta theta,
 *               P(t) = 1 + t (k1 + t (k2 + t (k3 + t k4))),  P'(t) = 1 + t (3 k1 + t (5 k2 + t (7 k3 + t 9 k4))),
 *               k = (theta P(t)) / rho,  u = (fx xc) k + cx,  v = (fy yc) k + cy
 *             zero coefficients give P = P' = 1 exactly: one code path, the plain fisheye is its zero-coefficient case.
 *   Position culls, ortho and fisheye only: a point with !(zc >= 0.01f) (render()'s near plane; NaN included) and, for a
 *   fisheye, one with P'(t) <= 0 (the fold, where the projection culls) is OUTSIDE, before any depth is read -- a centre the
 *   rasterizer never drew must not agree with whatever depth lies at the pixel it would land on.
 * The rendered depth is camera-space z for every model, so step 5 compares against zc unchanged.
 * cam_models: a HOST array of n_cams model ids, read completely before the call returns; NULL = all pinhole; an id outside the
 * three: GAGS_EINVAL before any launch.  radial_coeffs: a DEVICE array [n_cams, 4] or NULL (all zero); the rows of cameras
 * that are not fisheyes are not read.  Every other argument, the limits, the error codes and n == 0 are those of the two
 * entries above.  An all-pinhole rig (NULL or all ids 0) runs the very kernels of the entries above: the same bits.  The
 * scratch is a little larger than theirs (a wider camera block) and does not depend on the models. */
int64_t gags_rig_depth_scratch_bytes(int64_t n, int n_cams, int h, int w);
int gags_rig_depth_map(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats, const float *Ks,
                       const int32_t *cam_models, const float *radial_coeffs, const float *depths, float vis_thresh,
                       int cut_bound, float *min_depth, int32_t *mapping, unsigned char *visible, void *scratch,
                       int64_t scratch_bytes, void *stream);
int gags_rig_depth_scatter(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats, const float *Ks,
                           const int32_t *cam_models, const float *radial_coeffs, const float *depths, float vis_thresh,
                           int cut_bound, const float *min_depth, float *samples, void *scratch, int64_t scratch_bytes,
                           void *stream);

/* ---- N7: the photometric loss of the RGB stage (utils/loss_utils.py:20, 158-198; utils/image_utils.py:17-19) ------------
 * 3DGS's (1 - lambda) L1 + lambda (1 - SSIM) on images of `planes` = images x channels planes of h x w pixels, one forward and
 * one backward kernel (csrc/photometric.hip).  SSIM is the reference's: an 11 x 11 zero-padded window whose weight is the
 * product of two of the eleven taps `window` (a HOST array: the taps travel as kernel arguments; gags_amd.losses.SSIM_WINDOW),
 * moments mu1, mu2, E[x^2] - mu1^2, E[y^2] - mu2^2, E[xy] - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2 (as floats),
 *     map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)).
 * x, y and v_x are read and written through ELEMENT strides (plane, row, column): the rasterizer's [H, W, 3] memory is consumed
 * as it lies (strides 1, 3 W, 3), a contiguous [C, H, W] target through (H W, W, 1).  Strides must be >= 0 for x and y and
 * describe non-overlapping elements for v_x.  The filtered moments and everything derived from them are formed in double from
 * the float inputs (the subtraction E[x^2] - mu1^2 cancels on low-contrast windows); what is stored is float.
 *
 * Forward: every workgroup (a 32 x 16 tile of one plane) leaves three doubles in `partials`
 * [gags_photometric_partials(planes, h, w), 3]: sum of the map, sum |x - y|, sum (x - y)^2 over its pixels; no atomics.  One
 * more small launch adds them in a fixed order: sums[n_images, 3] (planes % n_images == 0; an image is planes / n_images
 * consecutive planes of n = that many h w elements) and, with r = sums / n per image (reduce_all = 0) or over everything
 * (reduce_all = 1: n = planes h w, one result),
 *     out[i] = bias + wa r[1] + wb r[0]   (float; photometric loss: bias = lambda, wa = 1 - lambda, wb = -lambda; SSIM: 0, 0, 1)
 *     k[0] = wa / n, k[1] = wb / n        (float; what the backward's coefficients are the cotangent's multiples of)
 * dm (optional) [3, planes, h, w]: the per-pixel partial derivatives of the map the backward filters -- d map / d mu1 (with the
 * mu-terms of the two below folded in), d map / d sigma1^2, d map / d sigma12.  ssim_map (optional) [planes, h, w]. */
int64_t gags_photometric_partials(int planes, int h, int w); /* host only; 0 for a shape the entries reject */
int gags_photometric_fwd(int planes, int n_images, int h, int w, const float *x, int64_t x_sp, int64_t x_sr, int64_t x_sc,
                         const float *y, int64_t y_sp, int64_t y_sr, int64_t y_sc, const float *window, double bias, double wa,
                         double wb, int reduce_all, float *dm, float *ssim_map, double *partials, double *sums, float *out,
                         float *k, void *stream);
/* Backward, one launch: v_x = a sign(x - y) + b (F[dm0] + 2 x F[dm1] + y F[dm2]) with F the same zero-padded filter (its own
 * adjoint), sign(0) = 0, and (a, b) = coef[image of the plane][0..1] read on the device (coef [n_images, 2] floats: the
 * cotangent times k, or one pair for everything when n_images = 1).  Written through v_x's strides. */
int gags_photometric_bwd(int planes, int n_images, int h, int w, const float *x, int64_t x_sp, int64_t x_sr, int64_t x_sc,
                         const float *y, int64_t y_sp, int64_t y_sr, int64_t y_sc, const float *window, const float *dm,
                         const float *coef, float *v_x, int64_t v_sp, int64_t v_sr, int64_t v_sc, void *stream);

/* ---- N8: adaptive density control (scene/gaussian_model.py:261-264, 321-482; train.py:206-218) ---------------------------
 * densify_and_prune as ONE plan and ONE gather (csrc/densify.hip).  Every clone, split and prune decision -- including whether
 * a split child survives the final prune -- depends only on the SOURCE Gaussian, so: decide (four flags per Gaussian), the
 * library's inclusive prefix sum on each flag array (K5; totals stay on the device), plan (source row and class of every output
 * row), gather (every tensor, once), children (positions and scales of the split children).  fp32, no FMA, IEEE division, no
 * atomics: bit-reproducible.  n = 0 (and an output of 0 rows) is accepted everywhere and launches nothing.
 *
 * Thresholds travel as floats: the reference compares a float32 tensor with a Python scalar, i.e. with the scalar rounded to
 * float32.  The caller forms percent_dense * extent and 0.1 * extent in double and rounds once.
 *
 * Statistics of one view (gaussian_model.py:476-482, train.py:209), one thread per Gaussian:
 *   u = update_filter[i] != 0 (NULL: radii[i] > 0):      accum[i] += sqrt(fl(gx half_w)^2 + fl(gy half_h)^2), denom[i] += 1
 *   v = visibility_filter[i] != 0 (NULL: radii[i] > 0):  max_radii[i] = max(max_radii[i], (float) radii[i])
 * with (gx, gy) = v_means2d[i, 0..1].  v_means2d NULL: only the radii update; max_radii NULL: only accum / denom. */
int gags_densify_stats(int n, const float *v_means2d, const int32_t *radii, const unsigned char *update_filter,
                       const unsigned char *visibility_filter, float half_w, float half_h, float *accum, float *denom,
                       float *max_radii, void *stream);
/* Decisions.  g = accum / denom with NaN -> 0 (x / 0 = inf stays), m = max_k exp(scaling[i, k]), o = sigmoid(opacity[i]):
 *   clone    = |g| >= max_grad and m <= dense_thr          split = g >= max_grad and m > dense_thr
 *   prune    = o < min_opacity or (use_screen and (0 > max_screen_size or m > world_thr))
 *   prune_ch = o < min_opacity or (use_screen and (0 > max_screen_size or m / 1.6f > world_thr))
 * (the screen-size test reads max_radii2D AFTER the clone step zeroed it: it compares zeros, as the reference does).
 * flags [4, n] int32: keeps itself = !split and !prune; clone survives = clone and !prune; split-selected = split;
 * children survive = split and !prune_ch. */
int gags_densify_decide(int n, const float *accum, const float *denom, const float *scaling, const float *opacity,
                        float max_grad, float dense_thr, float min_opacity, float world_thr, float max_screen_size,
                        int use_screen, int32_t *flags, void *stream);
/* Plan.  cum [4, n] = the inclusive prefix sums of the four flag rows, totals [4] (DEVICE) their sums (TK, TC, TS, TH); n_out =
 * TK + TC + 2 TH as the caller read it.  Output order: kept originals, surviving clones, surviving first children, surviving
 * second children, each in source order.  Per output row j: src[j] = source Gaussian, kind[j] = GAGS_KIND_*, zrow[j] = row of
 * the [2 TS, 3] normal samples a child uses = rank of its source among the split-selected (before pruning) + copy * TS
 * (-1 for rows that are no children).  Rows at or past n_out are not written. */
#define GAGS_KIND_KEEP 0
#define GAGS_KIND_CLONE 1
#define GAGS_KIND_CHILD_A 2
#define GAGS_KIND_CHILD_B 3
int gags_densify_plan(int n, const int32_t *flags, const int32_t *cum, const int32_t *totals, int64_t n_out, int32_t *src,
                      unsigned char *kind, int32_t *zrow, void *stream);
/* Gather, one launch for up to GAGS_GATHER_MAX_DESC tensors: out[j, :] = in[src[j], :] (COPY), or that for kind[j] == KEEP and
 * zeros otherwise (MOMENT: Adam's exp_avg / exp_avg_sq).  descs_host is a HOST array; rows are row_floats > 0 contiguous
 * floats.  16-byte lanes where row_floats % 4 == 0 and both bases are 16-byte aligned, 4-byte lanes otherwise; element offsets
 * are 64-bit (n_out row_floats may pass 2^31; n_out itself < 2^31).  src must index rows of `in`. */
#define GAGS_GATHER_MAX_DESC 24
#define GAGS_GATHER_COPY 0
#define GAGS_GATHER_MOMENT 1
typedef struct {
    const float *in;
    float *out;
    int32_t row_floats;
    int32_t mode;
} gags_gather_desc;
int gags_densify_gather(int64_t n_out, const int32_t *src, const unsigned char *kind, int n_desc,
                        const gags_gather_desc *descs_host, void *stream);
/* Children: rows j in [first_child, n_out) of xyz_out / scaling_out ([n_out, 3]; overwrites what the gather copied there), from
 * source i = src[j] (< n_src) and sample row k = zrow[j] (< n_z) of z [n_z, 3], in this order of operations:
 *   norm = sqrt(((w w + x x) + y y) + z z) of the STORED quaternion (w, x, y, z); q = stored / norm (four divisions)
 *   R = the matrix of utils/general_utils.py:78-99: R00 = 1 - 2 (y y + z z), R01 = 2 (x y - w z), R02 = 2 (x z + w y), ...
 *   t_a = exp(scaling[i, a]) * z[k, a]
 *   xyz_out[j, r] = ((R[r][0] t_0 + R[r][1] t_1) + R[r][2] t_2) + xyz[i, r]
 *   scaling_out[j, a] = log(exp(scaling[i, a]) / 1.6f)                                  (1.6f = fl32(0.8 * 2)) */
int gags_densify_children(int64_t n_out, int64_t first_child, int n_src, const int32_t *src, const int32_t *zrow,
                          const float *xyz_in, const float *scaling_in, const float *rotation_in, const float *z, int64_t n_z,
                          float *xyz_out, float *scaling_out, void *stream);
/* reset_opacity (gaussian_model.py:261-264), in place: x = min(sigmoid(o), 0.01f) (a NaN stays), o = log(x / (1 - x));
 * exp_avg / exp_avg_sq (each optional) = 0. */
int gags_reset_opacity(int64_t n, float *opacity, float *exp_avg, float *exp_avg_sq, void *stream);

/* ---- N9: scene initialisation from a point cloud (scene/gaussian_model.py:151-180 create_from_pcd; simple_knn distCUDA2) ------
 * dist2[i] = each point's mean squared distance to its three nearest neighbours.  The numerical contract: for point i, over all
 * j != i (excluded by INDEX, not by position: a duplicate point has distance 0 and counts as a neighbour),
 *   d2_ij = (dx*dx + dy*dy) + dz*dz,  dx = x_j - x_i (dy, dz likewise), float32, no FMA
 *   b0 <= b1 <= b2 = the three smallest d2_ij as VALUES
 *   dist2[i] = ((b0 + b1) + b2) / 3.0f                                    written in input order.
 * The multiset of the three smallest values does not depend on the visiting order: the result is bit-reproducible and
 * bit-equal to a float32 brute force (tests/knn_ref.py), whatever the traversal (csrc/knn.hip: Morton order, boxes of 256
 * sorted points pruned by a float32-exact lower bound).
 * n < 4 (the reference would give a point an infinite scale) or n >= 2^31: GAGS_EINVAL, nothing launched; the scratch size of
 * such an n is 0.  Non-finite coordinates give unspecified values (the call still terminates and stays inside its buffers).
 * xyz [n, 3] and dist2 [n] are device pointers; scratch is linear in n (about 44 n bytes). */
int64_t gags_knn3_dist2_scratch_bytes(int64_t n);
int gags_knn3_dist2(int64_t n, const float *xyz, float *dist2, void *scratch, int64_t scratch_bytes, void *stream);

/* ---- N10: SAM mask post-processing of the GAS stage (preprocess.py:373-489 mask_nms / filter / masks_update / mask2segmap,
 * :307-318 the level concatenation) on bit-packed masks (csrc/sam_masks.hip) ------------------------------------------------
 * masks[M, n_pixels]: one byte per pixel of the flattened row-major image, nonzero = set (torch bool and uint8 alike).
 * bits[M, nw] 64-bit words, nw = ceil(n_pixels / 64): pixel p is bit (p & 63) of word (p >> 6); the unused high bits of the
 * last word are zero.  area[M] int32 = set pixels per mask.
 *   inter[i, j] = sum_w popcount(bits[i, w] & bits[j, w])       int32, the full symmetric matrix; inter[i, i] = area[i]
 * (integer atomics into the matrix the entry zeroes: exact, order-independent; no float atomic anywhere in N10).
 * colmax[3, M] fp32 in mask_nms's arithmetic, over RANKS: order[M] lists the mask indices by descending score, a_i = area of
 * rank i, I = inter of the two ranks; counts converted to fp32, IEEE fp32 division, 1 - a b unfused, 0.5f and 0.85f:
 *   for i < j:  r_i = I / a_i,  r_j = I / a_j,  iou = I / (a_i + a_j - I)   (the union as an integer, then converted)
 *               inner[i, j] = 1 - r_j r_i  when r_i < 0.5 and r_j >= 0.85      (upper entry)
 *               inner[j, i] = 1 - r_j r_i  when r_i >= 0.85 and r_j < 0.5      (lower entry);  everything else 0
 *   colmax[0][c] = max(0, max_{i < c} iou[i, c])
 *   colmax[1][c] = max(0, max_{r < c} inner[r, c])
 *   colmax[2][c] = max(0, max_{r >= c - 1} inner[r, c])   (the reference's torch.tril(., diagonal=1): the first superdiagonal
 *                                                          belongs to the "lower" maximum too -- reproduced on purpose)
 * A zero-area mask makes its quotients NaN or inf; a NaN never wins a maximum, nothing else happens (the Python layer
 * refuses such a mask).  An entry of order or kept outside [0, M) is skipped.
 * paint: seg[n_pixels] int32 = offset + the largest k whose mask kept[k] covers the pixel, -1 where none does ("later paint
 * wins", mask2segmap); kept[n_kept] ascending mask indices, n_kept <= M, offset >= 0.  n_kept == 0: all -1.
 * Requires 1 <= n_pixels < 2^24 (beyond it the reference's float sums are no longer exact integers: no bit-exact contract)
 * and 0 <= M <= gags_masks_max_count() = 8192 (inter is M x M int32: 256 MiB at the cap, and i M + j stays far inside
 * int32).  M == 0: nothing is launched, GAGS_OK.  Every pointer is a device pointer. */
int gags_masks_max_count(void);
/* words of one mask that one block of the pair kernel reduces; more words than this are split across blocks */
int gags_masks_pair_chunk_words(void);
int gags_masks_pack(int n_masks, int64_t n_pixels, const unsigned char *masks, void *bits, int32_t *area, void *stream);
int gags_masks_pairs(int n_masks, int64_t n_pixels, const void *bits, int32_t *inter, void *stream);
int gags_masks_colmax(int n_masks, const int32_t *inter, const int32_t *area, const int32_t *order, float *colmax,
                      void *stream);
int gags_masks_paint(int n_masks, int64_t n_pixels, const void *bits, int n_kept, const int32_t *kept, int offset,
                     int32_t *seg, void *stream);
/* pack + pairs + colmax in one call: area[M] and colmax[3, M] out; bits and inter live in scratch (the _scratch_bytes()
 * bytes, 0 when M == 0) */
int64_t gags_masks_nms_scratch_bytes(int n_masks, int64_t n_pixels);
int gags_masks_nms_colmax(int n_masks, int64_t n_pixels, const unsigned char *masks, const int32_t *order, int32_t *area,
                          float *colmax, void *scratch, int64_t scratch_bytes, void *stream);

/* ---- N11: PCA colouring of a feature map (render.py:33-48 feature_visualize_saving; csrc/featurevis.hip) ------------------------
 * x is a [c, H, W] fp32 map of n_pix = H W pixels: layout 0 = channel-major (element (ch, p) at x[ch n_pix + p]), layout 1 =
 * pixel-major (x[p c + ch]: the memory behind the decoders' permuted view); neither is copied.  c % 16 == 0, 16 <= c <= 1024,
 * 1 <= n_pix <= 2^26.  x^ = x / max(||x||_2, 1e-12) per pixel (F.normalize).  The sample is every third pixel: p % 3 == 0,
 * S = ceil(n_pix / 3) of them.
 *   moments:  sum[c] = sum x^, gram[c, c] = sum x^ x^T over the sample, both float64 (S >= 4).  Exact-f32 matrix instructions
 *             on per-workgroup partial tiles (gags_featvis_row_chunk() sampled rows each), summed in float64 in a fixed order:
 *             two runs give the same bits.
 *   project:  t[p, k] = sum_ch (x^[ch] - mean[ch]) components[k, ch] for EVERY pixel, t [n_pix, 3]; mean [c], components [3, c].
 *   select:   out[j] = the ranks[j]-th smallest (0-based) of n pooled floats, exactly (two 16-bit histogram passes over
 *             order-preserving keys; -0.0 orders before +0.0).  Element i is values[(i / group) * stride + i % group]: group = 3,
 *             stride = 9 pools t's sampled rows.  `ranks` is a HOST array of n_ranks <= 8 values in [0, n); n < 2^31.
 *   colour:   vis[i] = clamp((t[i] - sub) / div, 0, 1) for n values; vis_u8 (optional) = trunc(255 vis[i]). */
int gags_featvis_row_chunk(void);
int64_t gags_featvis_moments_scratch_bytes(int c, int64_t n_pix);
int gags_featvis_moments(int c, int64_t n_pix, const float *x, int layout, double *sum, double *gram, void *scratch,
                         int64_t scratch_bytes, void *stream);
int gags_featvis_project(int c, int64_t n_pix, const float *x, int layout, const float *mean, const float *components, float *t,
                         void *stream);
int64_t gags_featvis_select_scratch_bytes(int n_ranks);
int gags_featvis_select(int64_t n, const float *values, int64_t group, int64_t stride, int n_ranks, const int64_t *ranks,
                        float *out, void *scratch, int64_t scratch_bytes, void *stream);
int gags_featvis_colour(int64_t n, const float *t, float sub, float div, float *vis, unsigned char *vis_u8, void *stream);

/* ---- N12: query images and loss maps (compute_relvancy.py:100-144 activate_stream --image_mode, the same images at
 * evaluate_iou_loc.py:108-163, 216-221; :439-447 compute_loss --loss_mode; csrc/queryvis.hip) --------------------------------------
 * Query images.  n_maps = frames x phrases maps of h x w pixels; heat (`blended`), output, mask (`mask_smooth`) and stats are
 * what gags_relevancy_activate wrote for them; image[n_frames, h, w, 3] fp32 in [0, 1], map m uses image m / (n_maps / n_frames);
 * lut[256, 3] fp32.  All arithmetic is fp32, one IEEE operation per step, no fused multiply-add.  Per map m and pixel p:
 *   idx(t)    = (int)(t * 255.0f) with a NaN t taken as 0, clamped to 0..255;  colour(t) = lut[idx(t)]   (eval/colormaps.py:105-113)
 *   heatmap_rgb = colour(output)                                                                          (:113, colormaps.py:69-80)
 *   lerf_rgb    = heat < 0.5f ? image * 0.3f : colour(q),   q = clip(p / (pmax + 1e-6f), 0, 1),           (:118-121)
 *                 p = clip(heat - 0.5f, 0, 1),  pmax = clip(stats[m][1] - 0.5f, 0, 1)
 *                 (stats[m][1] = max heat, and x -> clip(x - 0.5f, 0, 1) is monotone: pmax IS the reference's p.max(); no reduction)
 *   avg2        = the box x box mean of output by gags_relevancy_activate's rule for avg (anchor box / 2, BORDER_REFLECT_101,
 *                 sums in double, rounded once)                                                            (:136)
 *   mask_rgb    = mask ? colour(b) : (image * 0.4f) + 0.1f,   b = clip(0.5f * output + 0.5f * avg2, 0, 1)  (:138-142)
 *   *_u8 (optional: all three or none) = trunc(clamp(x * 255.0f + 0.5f, 0, 255)) of the float results: THIS project's 8-bit rule
 *                 (gags_amd/featurevis.py _save_image), declared here; the reference writes its PNGs through mediapy.
 * clip keeps a NaN (torch.clip), idx maps it to 0.  One thread per pixel, the LUT in LDS, grid (pixel blocks, n_maps): one launch
 * for every phrase of every frame; no atomics, results are bit-reproducible.
 * gags_query_colour: the colour kernel alone on a given avg2.  gags_query_images: the box mean of output into avg2[n_maps, h, w]
 * (scratch: the _scratch_bytes() bytes), then the colour kernel.
 * GAGS_EINVAL: a null pointer (the *_u8 excepted), a size <= 0, n_maps % n_frames != 0, box outside 1..1024, n_maps or h above
 * 65535; GAGS_ESCRATCH: scratch too small.  n_maps == 0 is a no-op. */
int64_t gags_query_images_scratch_bytes(int n_maps, int h, int w);
int gags_query_images(int n_maps, int n_frames, int h, int w, const float *heat, const float *output, const unsigned char *mask,
                      const float *stats, const float *image, const float *lut, int box, float *avg2, float *heatmap_rgb,
                      float *lerf_rgb, float *mask_rgb, unsigned char *heatmap_u8, unsigned char *lerf_u8, unsigned char *mask_u8,
                      void *scratch, int64_t scratch_bytes, void *stream);
int gags_query_colour(int n_maps, int n_frames, int h, int w, const float *heat, const float *output, const unsigned char *mask,
                      const float *avg2, const float *stats, const float *image, const float *lut, float *heatmap_rgb,
                      float *lerf_rgb, float *mask_rgb, unsigned char *heatmap_u8, unsigned char *lerf_u8, unsigned char *mask_u8,
                      void *stream);
/* Loss maps of compute_loss (:440-447).  feature and gt are maps of c channels x n_pix pixels, each in its own layout (0 =
 * channel-major x[ch n_pix + p], 1 = pixel-major x[p c + ch]); mask[n_pix] fp32 multiplies both.  Per pixel, with fl() one fp32
 * operation:  a = fl(gt * m), b = fl(feature * m), d = fl(a - b),
 *   l2 = sqrtf((float) sum_ch (double) fl(d * d)),  mean_abs_feature = (float)(sum_ch (double)|b| / c),  mean_abs_gt likewise of |a|.
 * The sums are accumulated in double and rounded once.  Their order is fixed by the channel index alone -- channel ch belongs to
 * run (ch % 64) / 16, every run is added in ascending channel order, and the four runs meet as (r0 + r1) + (r2 + r3) -- so any
 * combination of layouts gives the same bits.  Every element of both maps is read once, along its map's fast axis.
 * 1 <= c <= 65536, 0 <= n_pix <= 2^30 (0: a no-op). */
int gags_feature_loss_maps(int c, int64_t n_pix, const float *feature, int feature_layout, const float *gt, int gt_layout,
                           const float *mask, float *l2, float *mean_abs_feature, float *mean_abs_gt, void *stream);

/* ---- N13: crop statistics for SAM's depth-aware prompt grids (preprocess.py:114-149 build_depth_point_grid,
 * utils/SAM_utils.py:294-353 sample_based_mapping / build_mindepth_point_grid; csrc/promptgrid.hip) --------------------------
 * depths[C, h, w] fp32 (the rendered ED depth), samples[C, h, w] fp32 or NULL (N6's depth-sample maps), n = n_per_side.  Every
 * image is cut into n x n crops, crop k = ix n + iy (x outer: the order of itertools.product(crop_x0, crop_y0)).  The geometry
 * is integer and computed by the HOST in float64 exactly as numpy does (gags_amd/prompts.py crop_layout); the kernel never
 * evaluates a linspace.  tab (DEVICE, int32 [2 n + 20]) = x0[n], y0[n], sx[10], sy[10]:
 *   x0[i] = int32(linspace(0, w - 1, n + 1)[i]), crop_w = int(w / n); crop k covers columns [x0, min(x0 + crop_w, w)) and
 *   rows [y0, min(y0 + crop_h, h)): its shape (hc, wc).  Crops leave gaps when w % n != 0: that is the reference's grid.
 *   sx[j] = int32(linspace(0, wc - 1, 11)[j]), sy likewise of hc; sub-crop i (jx = i % 10, jy = i / 10) covers the crop's rows
 *   [sy[jy], min(hc - 1, sy[jy] + hc / 10)) and columns [sx[jx], min(wc - 1, sx[jx] + wc / 10)).  Neighbouring windows may share
 *   a pixel, a side under 10 gives empty windows, and the last row and column of a crop are in no window.
 * Outputs per camera c and crop k, [C, n n]:
 *   depth_sum float64 = sum of the crop's depths, depth_count int32 = hc wc;
 *   with samples: sample_sum float64 / sample_count int32 over the crop's samples != 0 (a NaN or a negative sample is
 *   non-zero, as for torch), sub_count[C, n n, 100] int32 = the non-zero samples in each sub-crop window.
 * The sums are float64 sums of the fp32 values in a fixed order (per-lane partials, a shuffle tree, the waves in order, row
 * slabs in ascending order; no floating-point atomics): equal inputs give equal bits.  The integer outputs are exact (the
 * sub-crop counters are integer LDS atomics: order-independent).  The kernel clamps every
 * start into the image and every window into its crop: no table can make it read outside the maps.
 * Crops are split into row slabs when C n n workgroups would not fill the chip (partials in scratch, a finishing step in a
 * fixed order).  scratch: the _scratch_bytes() bytes; 0 exactly when there is one slab and the workgroup writes the results.
 * GAGS_EINVAL: a size < 1, h w >= 2^31, n > 4096, crop_w / crop_h outside 0 .. w / h, C n n > 2^23, a null pointer (samples and
 * its three outputs excepted, together); GAGS_ESCRATCH: scratch too small. */
int64_t gags_promptgrid_scratch_bytes(int n_cams, int h, int w, int n_per_side, int crop_h);
int gags_promptgrid_stats(int n_cams, int h, int w, int n_per_side, int crop_w, int crop_h, const float *depths,
                          const float *samples, const int32_t *tab, double *depth_sum, int32_t *depth_count, double *sample_sum,
                          int32_t *sample_count, int32_t *sub_count, void *scratch, int64_t scratch_bytes, void *stream);

/* ---- N14: CLIP tiles from SAM masks (preprocess.py:356-371 get_seg_img / pad_img, :476-489 mask2segmap's tile cut with
 * cv2.resize(..., (224, 224)), :487 the float conversion; csrc/tilecut.hip) ------------------------------------------------------
 * image[H, W, 3] uint8, HWC as cv2.imread gives it.  bits[M, nw] exactly as gags_masks_pack writes them (N10): pixel
 * p = r W + c is bit (p & 63) of word (p >> 6).  index[K] int32 names the mask of each tile (any order, repeats allowed);
 * boxes[K, 4] int32 = (x, y, w, h), SAM's bbox.  bgr is 0 or 1.  All integer arithmetic below is exact.
 * Crop.  The box is clipped as a numpy slice clips it: w' = min(x + w, W) - x, h' = min(y + h, H) - y.  A tile whose box has
 *   x outside [0, W), y outside [0, H), w' < 1 or h' < 1, or whose index is outside [0, M), is written as all zeros (the Python
 *   layer raises ValueError instead); the kernel never reads outside image or bits.
 * Pad (pad_img, its `if h > w` / `else` exactly).  l = max(w', h'); ox = (l - w') / 2 when h' > w', else 0; oy = (l - h') / 2
 *   when h' <= w', else 0 (floor).  The square S[v, u, c], i = v - oy, j = u - ox:
 *     S[v, u, c] = image[y + i, x + j, c']  when 0 <= i < h', 0 <= j < w' and the mask's bit at pixel (y + i) W + x + j is set,
 *     S[v, u, c] = 0 otherwise;  c' = 2 - c when bgr (the reference's COLOR_BGR2RGB at :465), else c' = c.
 * Resize to 224 (8-bit INTER_LINEAR as OpenCV's generic path computes it; restated from memory, not pinned: DESIGN.md N14).
 *   scale = l / 224 in float64.  For d in 0 .. 223: f = (float)((d + 0.5) scale - 0.5) (a float64 product, then a float64
 *   subtraction, unfused); s = floor(f); f -= s (fp32); s < 0: s = 0, f = 0; s >= l - 1: s = l - 1, f = 0;
 *   a0 = rint((1.0f - f) * 2048.0f), a1 = rint(f * 2048.0f) (nearest even); taps s and min(s + 1, l - 1).  One table for both
 *   axes.  Horizontal: h = S0 a0 + S1 a1 (int).  Vertical: out = ((b0 (h0 >> 4) >> 16) + (b1 (h1 >> 4) >> 16) + 2) >> 2.
 *   l = 224 is the identity and l = 448 the 2 x 2 mean (s00 + s01 + s10 + s11 + 2) >> 2 (where OpenCV switches to its area
 *   path): the arithmetic above gives both.
 * Outputs: tiles_u8[K, 224, 224, 3]; tiles_f32[K, 3, 224, 224] = (float)u8 / 255.0f by an IEEE division (torch's
 *   x.float() / 255.0 on the host, where preprocess.py:487 divides, bit for bit; on a GPU tensor torch multiplies by the
 *   rounded reciprocal instead).  Either may be NULL, not both.  Output offsets are 64-bit.
 * gags_tilecut_boxes (named outside gags_masks_*, N10's closed set of eight entries): boxes[M, 4] int32 = (x0, y0, x1, y1), the
 *   inclusive tight bounds of every mask's set pixels; an empty mask gives (0, 0, -1, -1).  Bits at or beyond pixel H W are
 *   ignored.
 * Limits are N10's: 1 <= H W < 2^24 and 0 <= K, M <= gags_masks_max_count(); a count of 0 launches nothing (gags_tilecut with
 * K > 0 needs M >= 1).  GAGS_EINVAL otherwise, for bgr outside {0, 1} and for a null pointer, before any launch.  No atomics;
 * every pointer is a device pointer. */
int gags_tilecut_side(void);
int gags_tilecut(int n_tiles, int height, int width, const unsigned char *image, int bgr, int n_masks, const void *bits,
                 const int32_t *index, const int32_t *boxes, unsigned char *tiles_u8, float *tiles_f32, void *stream);
int gags_tilecut_boxes(int n_masks, int height, int width, const void *bits, int32_t *boxes, void *stream);

/* ---- N15: the query head -- phrase relevancy straight from the rasterized features (evaluate_iou_loc.py:258-288,
 * compute_relvancy.py:243-269, 333-361; csrc/decoder_query.hip) ---------------------------------------------------------------
 * One forward-only kernel:  x[n_pix, c_in] fp32 (pixel-major, the rasterizer's layout) -> CNN_decoder's nine layers per
 * 64-pixel tile in LDS, arithmetic and bits of gags_decoder_fwd_fused (same operands: w_bf16[9] in MFMA-fragment order, bias[9]
 * padded fp32) -> fp32 logits z[n_last] per pixel, which never leave the chip ->
 *     sim_j = z . t_j / max(||z||, 1e-12)     for the n_pos + n_neg rows t_j of phrases[n_pos + n_neg, n_last] (fp32, positives
 *                                             first, 16-byte aligned; unit rows, as OpenCLIPNetwork holds them)
 *     probs[j, pixel, 0..1] = softmax(10 (sim_j, sim_(n_pos + k)))  of the negative k with the smallest first component (the
 *                                             first such k), for every positive j:  gags_relevancy's output, probs[n_pos, n_pix, 2].
 * Equal to gags_decoder_fwd_fused -> gags_decoder_head (normalize) -> gags_relevancy up to fp32 summation order; nothing but
 * probs is written.  n_pix == 0 launches nothing.  GAGS_EINVAL: n_pix < 0, c_in outside 1 .. 32, n_last <= 0 or not a multiple
 * of 256, n_pos <= 0, n_neg <= 0, n_pos + n_neg > 32 (gags_relevancy's cap), a null pointer (x and probs may be null when
 * n_pix == 0), misaligned phrases / probs. */
int gags_decoder_query_fused(int64_t n_pix, int c_in, int n_last, const float *x, const void *const *w_bf16,
                             const float *const *bias, const float *phrases, int n_pos, int n_neg, float *probs, void *stream);

/* ---- N18: MCMC density control ("3D Gaussian Splatting as Markov Chain Monte Carlo": relocation, capped growth, position
 * noise; csrc/mcmc.hip, gags_amd/mcmc.py; the rules R1-R6 are declared in DESIGN.md section 7 "N18") -------------------------
 * Stored parameters as everywhere: opacity [n] logits, scaling [n, 3] logs, rotation [n, 4] (w, x, y, z) un-normalised,
 * xyz [n, 3]; fp32, contiguous.  n = 0 (and zero draws / pairs) is accepted everywhere and launches nothing.  No float atomics,
 * no inline assembly: two runs give the same bits.
 *
 * Sampling (R2).  cdf [n] float64 = the inclusive prefix sums of non-negative weights (non-decreasing), u [n_draws] float64 in
 * [0, 1).  One thread per draw: t = u * cdf[n - 1]; draws[k] = the first j with cdf[j] > t (binary search), and when no entry
 * exceeds t the first j with cdf[j] == cdf[n - 1]: a row of weight zero (cdf[j] == cdf[j - 1]) is never drawn.
 * counts[j] += 1 per draw of j (int32 atomics: exact, order-free); the CALLER zero-fills counts [n] first.
 * GAGS_EINVAL: n < 0, n_draws < 0 or >= 2^31, n == 0 with n_draws > 0, a null pointer while n_draws > 0. */
int gags_mcmc_sample(int n, const double *cdf, int64_t n_draws, const double *u, int32_t *draws, int32_t *counts, void *stream);
/* Relocation values (R1), in place, over the rows with k[i] > 0; every other row is not touched.  r = k[i] + ratio_bias clamped
 * to [1, GAGS_MCMC_MAX_RATIO] (ratio_bias 1: k = gags_mcmc_sample's counts; ratio_bias 0: k = the ratios themselves).  Per row,
 * in FLOAT64 from the stored float32 values, rounded once at the end:
 *   q     = max(1 / (1 + exp(x)), 2^-23),  o = 1 - q                      (x the logit: o = min(sigmoid(x), 1 - 2^-23))
 *   o_new = 1 - q^(1/r)                                                   (as -expm1(log(q) / r))
 *   denom = sum_{i = 1..r} sum_{k = 0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1)      (in this order; C from a constant
 *                                                                          51 x 51 table of exact doubles)
 *   scaling[i, a] = fl32(scaling[i, a] + log(o / denom))   a = 0, 1, 2;   r == 1: not written (o_new = o, the coefficient is 1)
 *   opacity[i]    = fl32(logit(min(max(o_new, min_opacity), 1 - 2^-23)))
 * GAGS_EINVAL: n < 0, ratio_bias outside {0, 1}, min_opacity outside (0, 1) (a NaN included), a null pointer while n > 0. */
#define GAGS_MCMC_MAX_RATIO 51
int gags_mcmc_relocation(int n, const int32_t *k, int ratio_bias, double min_opacity, float *opacity, float *scaling,
                         void *stream);
/* Row copies of a relocation (R3) for up to GAGS_GATHER_MAX_DESC tensors of n_rows rows in one launch, IN PLACE (gags_gather_desc
 * with in == out, rows of row_floats > 0 floats, 16-byte lanes as for gags_densify_gather), over the n_pairs pairs
 * (dst_rows[p] int64, src_rows[p] int32):
 *   GAGS_GATHER_COPY:    out[dst_rows[p], :] = out[src_rows[p], :]       (bit copies; the caller keeps the two sets disjoint)
 *   GAGS_GATHER_MOMENT:  out[src_rows[p], :] = 0                          (Adam's moments at the drawn sources; dst rows keep theirs)
 * A pair with a row outside [0, n_rows) is skipped.  GAGS_EINVAL: n_pairs < 0 or >= 2^31, n_rows < 0, n_desc outside
 * [0, GAGS_GATHER_MAX_DESC], a descriptor with in != out, a null pointer, row_floats <= 0 or an unknown mode, null row lists
 * while there is work. */
int gags_mcmc_copy_rows(int64_t n_pairs, const int64_t *dst_rows, const int32_t *src_rows, int n_rows, int n_desc,
                        const gags_gather_desc *descs_host, void *stream);
/* Position noise (R5), one thread per Gaussian, fp32, no FMA, xyz in place (68 bytes of traffic per Gaussian):
 *   o = 1 / (1 + exp(-x)),  gate = 1 / (1 + exp(-100 ((1 - o) - 0.995f)))
 *   norm = sqrt(((w w + x x) + y y) + z z), q = stored / norm, R as gags_densify_children builds it, M[r][a] = R[r][a] exp(s_a)
 *   S[r][c] = (M[r][0] M[c][0] + M[r][1] M[c][1]) + M[r][2] M[c][2]
 *   v_a = (z[i, a] * gate) * scaler,   xyz[i, r] += (S[r][0] v_0 + S[r][1] v_1) + S[r][2] v_2
 * GAGS_EINVAL: n < 0, a null pointer while n > 0, scaler not finite. */
int gags_mcmc_noise(int n, const float *opacity, const float *scaling, const float *rotation, const float *z, float scaler,
                    float *xyz, void *stream);
/* Regularisers (R6): out[0] = opacity_reg mean(sigmoid(opacity)) + scale_reg mean(exp(scaling)) (means over n and 3 n entries).
 * Per element in float64; a fixed-order float64 tree over the 64 lanes of a wave, the four wave sums of a workgroup added in
 * wave order, fl32(opacity_reg / n * sum_o + scale_reg / (3 n) * sum_s) as the workgroup's row of `partials`, then
 * gags_colsum_f32 over the rows: deterministic.  partials: gags_mcmc_reg_partials(n) floats (partials_bytes >= 4 * that, else
 * GAGS_EINVAL before any launch).  n = 0: out[0] = 0.
 * Backward, one launch, closed form, float64 per element rounded once; g = v_out[0], a DEVICE float (no host sync):
 *   v_opacity[i] = g opacity_reg / n * o (1 - o),   v_scaling[i, a] = g scale_reg / (3 n) * exp(s_a)
 * GAGS_EINVAL: n < 0, a null pointer (partials and the inputs may be null when n == 0), coefficients not finite. */
int64_t gags_mcmc_reg_partials(int n);
int gags_mcmc_reg_fwd(int n, const float *opacity, const float *scaling, float opacity_reg, float scale_reg, float *partials,
                      int64_t partials_bytes, float *out, void *stream);
int gags_mcmc_reg_bwd(int n, const float *opacity, const float *scaling, float opacity_reg, float scale_reg, const float *v_out,
                      float *v_opacity, float *v_scaling, void *stream);

/* ---- the "f16" decoder tier -------------------------------------------------------------------------------------------
 * The SAME kernels compiled with IEEE half as their 16-bit operand type (csrc/half16.h; v_mfma_f32_32x32x16_f16, fp32
 * accumulation): an 11-bit significand -- exactly the TF32 significand the reference's nn.Conv2d layers
 * (models/networks.py:145-149,229-233) compute with under PyTorch's default torch.backends.cudnn.allow_tf32 = True --
 * instead of bfloat16's 8.  Same signatures and semantics as the entry points above; every `*_bf16` pointer is a half
 * tensor.  Half has 5 exponent bits: conversions saturate at +-65504 (never inf), and the caller multiplies the gradient
 * entering a backward chain by a power of two (gags_amd/decoders.py does: precision="f16") and divides the results. */
/* The tier's gradient scale from the cotangent's magnitude, on the device: out[0] = S = 2^floor(target_log2 - log2(amax[0] / div))
 * (exponent clamped to +-100; S = 1 when amax is 0 or not finite), out[1] = 1 / S. */
int gags_pow2_scale(const float *amax, float div, float target_log2, float *out, void *stream);
int gags_decoder_pack_layer_h16(int co, int ci, const float *w, const float *b, void *w_bf16, void *wt_bf16, void *w_frag, void *wt_frag, float *bias_pad, void *stream);
int gags_decoder_pack_layers_h16(int n_layers, const int *co, const int *ci, const float *const *w, const float *const *b, void *const *w_bf16, void *const *wt_bf16, void *const *w_frag, void *const *wt_frag, float *const *bias_pad, void *stream);
int gags_decoder_pack_input_h16(int64_t n_pix, int c, int c_pad, const float *x, void *y_bf16, void *stream);
int gags_decoder_layer_h16(int64_t n_pix, int n_out, int k_in, const void *a1, const void *a2, const void *w, const float *bias, int relu, const void *mask_src, const void *residual, void *y_bf16, void *y_premask_bf16, float *y_f32, void *stream);
int gags_decoder_head_h16(int64_t n_pix, int c, int ld, int mode, const float *x, float *out, int layout, void *stream);
int64_t gags_decoder_wgrad_scratch_bytes_h16(int64_t n_pix, int n_out, int k_in);
int gags_decoder_wgrad_h16(int64_t n_pix, int n_out, int k_in, const void *dz, const void *a1, const void *a2, float *d_w, float *d_b, void *scratch, int64_t scratch_bytes, void *stream);
int gags_decoder_wgrad_out_h16(int64_t n_pix, int n_out, int k_in, const void *dz, const void *a1, const void *a2, float *d_w, float *d_b, int co, int ci, const float *out_scale, void *scratch, int64_t scratch_bytes, void *stream);
int gags_decoder_head_bwd_h16(int64_t n_pix, int c, int ld, int mode, const float *x, const float *g, void *dz_bf16, int layout, void *stream);
int gags_decoder_unpack_grad_h16(int64_t n_pix, int c, int ld, const void *x_bf16, float *y, void *stream);
int gags_decoder_fwd_fused_h16(int64_t n_pix, int c_in, int n_last, const float *x, const void *const *w_bf16, const float *const *bias, void *const *acts_bf16, void *masks, float *logits, void *stream);
int gags_decoder_bwd_fused_h16(int64_t n_pix, int c_in, int n_last, const void *dz_last_bf16, const void *const *wt_bf16, const void *masks, void *const *dz_bf16, float *gin, void *stream);
int gags_decoder_bwd_fused_scaled_h16(int64_t n_pix, int c_in, int n_last, const void *dz_last_bf16, const void *const *wt_bf16, const void *masks, void *const *dz_bf16, float *gin, const float *gin_scale, void *stream);
int gags_scale_decoder_bwd_fused_h16(int64_t n_pix, const void *dz_last_bf16, const void *const *wt_bf16, const void *masks, void *const *dz_bf16, void *stream);
/* the fused head + distillation L1 backward (gags_decoder_head_distill_bwd) with the logits' gradient as IEEE half, multiplied by
 * the power of two dz_scale[0] (a DEVICE float: chosen by the caller without a host sync) and saturated at +-65504 */
int gags_decoder_head_distill_bwd_h16(int c, int ld, int H, int W, int h, int w, int n_emb, const float *x,
                                     const float *img_embed, const float *seg_map, const float *scale_map,
                                     const float *v_map, void *dz_f16, const float *dz_scale, float *v_scale, void *stream);
int gags_scale_decoder_fwd_fused_h16(int64_t n_pix, int c_in, const float *x, const void *const *w_bf16, const float *const *bias, void *const *acts_bf16, void *masks, float *logits, void *stream);
int gags_scale_decoder_fwd_fused_head_h16(int64_t n_pix, int c_in, const float *x, const void *const *w_bf16, const float *const *bias, void *const *acts_bf16, void *masks, float *logits, float *softmax3, void *stream);
int gags_softmax_head_bwd_y_h16(int64_t n_pix, int c, int ld, const float *y, const float *g, void *dz_bf16, void *stream);
int gags_decoder_query_fused_h16(int64_t n_pix, int c_in, int n_last, const float *x, const void *const *w_bf16, const float *const *bias, const float *phrases, int n_pos, int n_neg, float *probs, void *stream);

/* ---- N24: bilateral grid colour correction (csrc/bilagrid.hip) -------------------------------------------------------------
 * A grid g [12, L, gh, gw] of floats holds a 3 x 4 colour transform per node: channel 4 r + c is entry (r, c), columns 0..2
 * multiply (R, G, B), column 3 is the bias.  For pixel (row i, column j) of an h x w image with colour p = (R, G, B):
 *     x = ((j + 0.5) / w) (gw - 1),  y = ((i + 0.5) / h) (gh - 1),
 *     gray = 0.299 R + 0.587 G + 0.114 B,  z = clamp(gray, 0, 1) (L - 1),
 *     A[ch] = sum_{l, m, n} g[ch, l, m, n] tent(z - l) tent(y - m) tent(x - n),   tent(t) = max(0, 1 - |t|),
 *     out[r] = A[r, 0] R + A[r, 1] G + A[r, 2] B + A[r, 3]
 * -- torch.nn.functional.grid_sample(mode "bilinear", align_corners = True, padding_mode "border") at (2 x / (gw - 1) - 1,
 * 2 y / (gh - 1) - 1, 2 gray - 1).  Backward: v_g is the adjoint of the sum;
 *     v_p[c] = sum_r A[r, c] v_out[r] + m (L - 1) w_c sum_ch (dA[ch] / dz) v_out[r(ch)] (p, 1)[c(ch)],
 * m = 1 where 0 < gray (L - 1) < L - 1 and 0 otherwise (no gradient through a clamped or boundary coordinate; exact black is
 * one), d / dz taken in the cell [floor z, floor z + 1]; x and y are constants.
 * Supported: 2 <= L <= 16, 2 <= gh, gw <= 64, h, w >= 1 with h w <= 2^30; anything else, a NULL pointer or a negative
 * stride is GAGS_EINVAL before any launch.  rgb and v_out are read through ELEMENT strides (plane, row, column): the
 * rasterizer's [h, w, 3] memory is (1, 3 w, 3), a contiguous [3, h, w] is (h w, w, 1).  out and v_rgb are [h, w, 3] memory.
 * Backward: v_rgb and v_grid are each optional (not both NULL).  v_grid [12, L, gh, gw] is computed without atomics and is
 * bit-reproducible: a workgroup per (xy-node, chunk of the node's rows) gathers its pixels into registers and stores its
 * sums into one of the scratch's slabs, a second kernel adds the slabs in order; every element is written, nodes no pixel
 * reaches as 0.  scratch (needed for v_grid only): gags_bilagrid_scratch_bytes(L, gh, gw) bytes, less is GAGS_ESCRATCH. */
int64_t gags_bilagrid_scratch_bytes(int L, int gh, int gw); /* host only; 0 for a grid the entries reject */
int gags_bilagrid_slice_fwd(int L, int gh, int gw, int h, int w, const float *grid, const float *rgb, int64_t sp, int64_t sr,
                            int64_t sc, float *out, void *stream);
int gags_bilagrid_slice_bwd(int L, int gh, int gw, int h, int w, const float *grid, const float *rgb, int64_t sp, int64_t sr,
                            int64_t sc, const float *v_out, int64_t v_sp, int64_t v_sr, int64_t v_sc, float *v_rgb,
                            float *v_grid, void *scratch, int64_t scratch_bytes, void *stream);
/* Total variation of grids [n_images, 12, L, gh, gw]:
 *     tv = (2 / n_images) sum_{d in (L, gh, gw)} sum (g[.. d + 1 ..] - g[.. d ..])^2 / n_d,
 * n_d the number of differences of ONE image along d (12 (L - 1) gh gw for d = L, and so on).  Forward: the differences and
 * their squares in double, three doubles per workgroup in partials [gags_bilagrid_tv_partials(...), 3], added in a fixed order
 * by one more workgroup; out [1] float.  Backward: v_grids = v[0] (4 / (n_images n_d)) (second difference), v a DEVICE float.
 * 1 <= n_images <= 65536. */
int64_t gags_bilagrid_tv_partials(int n_images, int L, int gh, int gw); /* host only; 0 for sizes the entries reject */
int gags_bilagrid_tv_fwd(int n_images, int L, int gh, int gw, const float *grids, double *partials, float *out, void *stream);
int gags_bilagrid_tv_bwd(int n_images, int L, int gh, int gw, const float *grids, const float *v, float *v_grids, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* GAGS_NEXT_H */
