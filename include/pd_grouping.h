/*
 * pd_grouping.h — C-ABI of the pixel-grouping (part-proposal generation) kernel of libpd_hip.so.
 *
 * Reference: proposal_generation_model.py:131-146 + 224-237 (twin: pixel_grouping_model.py:183-218).  The reference
 * upsamples the C-channel backbone features of an image to full resolution ([C, H, W] fp32: 4.8-6.4 GB per 1024^2 image),
 * gathers the object's pixels, ships them to the CPU and takes argmax_k of `feature . centroid_k` (metric "dot") or of
 * `2 feature . centroid_k - |feature|^2 - |centroid_k|^2` (metric "l2").  Bilinear interpolation is linear with weights
 * that sum to one, so the per-centroid scores  s_k = F . c_k  (dot)  /  2 F . c_k - |c_k|^2  (l2; the -|feature|^2 term
 * is the same for every k) can be formed at feature resolution ([K, h, w], K = 4) and interpolated instead:
 * ~1 MB of label map per image instead of gigabytes of features.
 */
#ifndef PD_GROUPING_H
#define PD_GROUPING_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * labels[y, x] (uint8, [H, W]) = mask[y, x] ? 1 + argmax_k bilinear(scores_k)(y, x) : 0          (first maximum wins)
 * scores: fp32 [K, h, w] of one image (K <= 32); bilinear = F.interpolate(size=(Hp, Wp), mode="bilinear",
 * align_corners=False) evaluated on the top-left H x W crop (H <= Hp, W <= Wp: the un-padded image);
 * mask: uint8 [H, W] (nonzero = object pixel).
 */
int pd_scores_argmax_u8(const float *scores, const uint8_t *mask, uint8_t *labels, int K, int h, int w, int Hp, int Wp, int H,
                        int W, void *stream);

/*
 * Per-pixel assignment of the K selected query masks at inference (reference proposal_model.py:220-302:
 * F.interpolate of [Q, H/4, W/4] logits to the padded image size, `* object mask` (:372-378), `_unique_assignment`
 * :263-299).  The reference materialises [Q, H, W] fp32 three times (0.4 GB per image and copy at 1024^2, Q = 100);
 * here the low-resolution logits (26 MB) are interpolated inside the one pass that consumes them:
 *   v_k   = bilinear(logits_k)(y, x) * (object ? object[y, x] != 0 : 1)
 *   arg   = argmax_k scores[k] * sigmoid(v_k)   (first maximum)              int16 [H, W]
 *   obj   = max_k v_k > 0                                                     uint8 [H, W]
 *   positive[k] += #pixels with v_k > 0         (int32 [K], caller zeroes)
 * logits fp32 [K, h, w]; bilinear as in pd_scores_argmax_u8 (upsample to (Hp, Wp), top-left H x W crop).
 */
int pd_mask_assign(const float *logits, const float *scores, const uint8_t *object, int16_t *arg, uint8_t *obj, int32_t *positive,
                   int K, int h, int w, int Hp, int Wp, int H, int W, void *stream);

/*
 * Evaluation twin (reference pixel_grouping_model.py:129-218): the data mapper has resized the image, so every full-resolution map goes
 * through detectron2's sem_seg_postprocess — crop the padding, then a second bilinear resize to the output size.  Both kernels below
 * serve ALL images of a batch in ONE launch: the caller passes a host list of descriptors, a pinned staging buffer and a device buffer
 * of pd_grouping_table_bytes(count) bytes each (the pinned one must stay untouched until the asynchronous copy has executed).
 *
 * Both resizes are F.interpolate(mode="bilinear", align_corners=False) with ATen's fp32 index rule, every operation rounded on its own:
 *   scale = (float)in / out;  src = max(scale * (dst + 0.5f) - 0.5f, 0);  i0 = (int)src;  i1 = i0 + (i0 < in - 1);
 *   l1 = src - i0;  l0 = 1 - l1.
 */
#define PD_GROUPING_MAX_K 32

int64_t pd_grouping_table_bytes(int32_t count);

/*
 * labels[y, x] (uint8 [H, W]) = mask[y, x] ? 1 + argmax_k S2_k(y, x) : 0                          (first maximum wins)
 *   S2_k = bilinear((Hi, Wi) -> (H, W))( crop[:Hi, :Wi]( bilinear((h, w) -> (Hp, Wp))(scores_k) ) )
 * The second interpolation clamps its taps at the crop's edge (Hi - 1, Wi - 1).  Interpolation is linear, so an output pixel is a
 * separable combination of at most 4 x 4 samples of scores_k: neither [K, Hp, Wp] nor [K, H, W] is ever written.
 * counts[l] (int32 [K + 1], zero on entry) += number of pixels given label l, 0 included: the bincount of the label map.
 * scores fp32 [K, h, w] contiguous, 1 <= K <= PD_GROUPING_MAX_K; mask uint8 [H, W] (non-zero = object); 0 < Hi <= Hp, 0 < Wi <= Wp.
 * For (H, W) == (Hi, Wi) the second interpolation is the identity and the labels are those of pd_scores_argmax_u8.
 */
typedef struct PdGroupLabels {
  const float *scores;
  const uint8_t *mask;
  uint8_t *labels;
  int32_t *counts;
  int32_t K, h, w, Hp, Wp, Hi, Wi, H, W;
  int32_t reserved;
} PdGroupLabels;
int pd_scores_argmax_resized_u8(const PdGroupLabels *list, int32_t count, void *table_host_pinned, void *table_device, void *stream);

/*
 * dst (uint8 [n, H, W], 0 / 1) = bilinear((Hi, Wi) -> (H, W))( crop[:Hi, :Wi](src != 0 as float) ) != 0 for n masks of one image:
 * `sem_seg_postprocess(masks, image_size, H, W).bool()`.  Every weight is >= 0, so a pixel is set exactly when one of its 2 x 2 taps
 * WITH A NON-ZERO WEIGHT (l0 > 0 always; l1 == 0 when src is an integer) is set: no float image exists.
 * area[i] (int64 [n], zero on entry) += set pixels of dst[i].  src uint8 [n, Hp, Wp] contiguous; n == 0 is a no-op.
 */
typedef struct PdMaskResize {
  const uint8_t *src;
  uint8_t *dst;
  int64_t *area;
  int32_t n, Hp, Wp, Hi, Wi, H, W;
  int32_t reserved;
} PdMaskResize;
int pd_masks_resize_u8(const PdMaskResize *list, int32_t count, void *table_host_pinned, void *table_device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_GROUPING_H */
