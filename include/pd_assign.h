/*
 * pd_assign.h — C-ABI of the per-pixel mask assignment at a RESIZED output and of its histogram (csrc/mask_assign_resized.hip).
 *
 * Reference: supervised_model.py:201-335.  Evaluation mappers resize the image, so the output size (height, width) differs from the size
 * the network saw and every full-resolution map goes through detectron2's sem_seg_postprocess (crop the padding, second bilinear resize).
 * The reference does that to all Q mask-logit maps ([Q, H, W] fp32, twice), multiplies by the object mask, takes sigmoid, scales by the
 * scores and arg-maxes; the IoUs with the ground-truth parts then need one pass over the map per mask.  Here one kernel interpolates the
 * low-resolution logits twice inside the pass that consumes them, and one kernel counts everything the matching needs in one pass.
 *
 * pd_pair_assign_resized is the assignment for (query, class) pairs that share logit maps (the class-aware branches of inference.py).
 *
 * Every kernel serves ALL images of a batch in ONE launch: the caller passes a host list of descriptors, a pinned staging buffer and a
 * device buffer of pd_assign_table_bytes(count) bytes each (the pinned one must stay untouched until the asynchronous copy has
 * executed).  All other pointers are device pointers; `stream` = hipStream_t; returns 0 or PD_ERR_* (pd_msda.h) with pd_last_error() set.
 * Nothing is launched when a descriptor is invalid.
 */
#ifndef PD_ASSIGN_H
#define PD_ASSIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_ASSIGN_MAX_K 256           /* selected queries per image (TEST.DETECTIONS_PER_IMAGE) */
#define PD_ASSIGN_MAX_Q 1024          /* queries that the pairs of pd_pair_assign_resized refer to */
#define PD_ASSIGN_MAX_KEYS 1024      /* keys of pd_assign_histogram (queries or classes) */
#define PD_ASSIGN_MAX_GT 64           /* ground-truth masks per image (= PD_EVAL_MAX_GT) */

int64_t pd_assign_table_bytes(int32_t count);

/*
 * pd_mask_assign (pd_grouping.h) for an output that goes through sem_seg_postprocess:
 *   v_k  = bilinear((Hi, Wi) -> (H, W))( crop[:Hi, :Wi]( bilinear((h, w) -> (Hp, Wp))(logits_k) ) )(y, x) * (object ? object[y, x] != 0 : 1)
 *   arg  = argmax_k scores[k] * sigmoid(v_k)      (first maximum)                int16 [H, W]
 *   obj  = max_k v_k > 0                                                          uint8 [H, W]
 *   positive[k] += #pixels with v_k > 0           (int32 [K], zero on entry)
 *   cls  = obj ? cls_of_query[arg] : -1           (only when cls_of_query and cls are given)    int16 [H, W]
 * Both interpolations are F.interpolate(mode="bilinear", align_corners=False) with ATen's fp32 index rule, every operation rounded on
 * its own (pd_grouping.h); the second clamps its taps at the crop's edge.  An output pixel is a separable combination of at most 4 x 4
 * samples of logits_k: neither [K, Hp, Wp] nor [K, H, W] is ever written.
 * logits fp32 [K, h, w] contiguous, 1 <= K <= PD_ASSIGN_MAX_K (PD_ERR_INVALID_ARG above); scores fp32 [K]; object nullable uint8 [H, W];
 * cls_of_query nullable int32 [K] with values in [-1, 32767]; 0 < Hi <= Hp, 0 < Wi <= Wp.
 * For (H, W) == (Hi, Wi) the second interpolation is the identity, and the kernel then evaluates v_k with the very expression of
 * pd_mask_assign: arg, obj and positive are bit-identical to its results.
 */
typedef struct PdAssignResized {
  const float *logits;
  const float *scores;
  const uint8_t *object;
  const int32_t *cls_of_query;
  int16_t *arg;
  uint8_t *obj;
  int32_t *positive;
  int16_t *cls;
  int32_t K, h, w, Hp, Wp, Hi, Wi, H, W;
  int32_t reserved;
} PdAssignResized;
int pd_mask_assign_resized(const PdAssignResized *list, int32_t count, void *table_host_pinned, void *table_device, void *stream);

/*
 * pd_mask_assign_resized for K (query, class) PAIRS that share queries: the class-aware evaluation branches select the top K of the
 * Q x nc scores, so several pairs read one mask-logit map.  Pair k stands for logits[pair_query[k]]; every output is bit-identical to
 * pd_mask_assign_resized run on the gathered stack logits[pair_query] (first maximum in pair order, the identity-size branch and
 * segments without an object pixel included), but no [K, h, w] copy is made and a workgroup interpolates every REFERENCED query once
 * (row mix, the 4 x 4 taps, the sigmoid) and then walks that query's pairs for the products scores[k] * sigmoid(v).
 * logits fp32 [Q, h, w] contiguous, 1 <= Q <= PD_ASSIGN_MAX_Q; pair_query int32 [K] (device) with values in [0, Q): the range is the
 * caller's contract (a pair outside it never wins a pixel and counts nothing); scores fp32 [K]; cls_of_pair nullable int32 [K] with
 * values in [-1, 32767]; object nullable uint8 [H, W]; arg int16 [H, W] holds the PAIR index; positive int32 [K] (zero on entry):
 * positive[k] += #pixels with v > 0 for the query of pair k; cls = obj ? cls_of_pair[arg] : -1.  1 <= K <= PD_ASSIGN_MAX_K.
 */
typedef struct PdAssignPairs {
  const float *logits;
  const int32_t *pair_query;
  const float *scores;
  const int32_t *cls_of_pair;
  const uint8_t *object;
  int16_t *arg;
  uint8_t *obj;
  int32_t *positive;
  int16_t *cls;
  int32_t K, Q, h, w, Hp, Wp, Hi, Wi, H, W;
} PdAssignPairs;
int pd_pair_assign_resized(const PdAssignPairs *list, int32_t count, void *table_host_pinned, void *table_device, void *stream);

/*
 * One pass over an assignment map `key` (arg, or cls: int16 [hw]), its object map and the G ground-truth masks (uint8 [G, hw]):
 *   won[k]      += #(key == k)                       (the reference's scoremap.unique(): the keys with won > 0)
 *   area[k]     += #(key == k & obj)
 *   inter[k][j] += #(key == k & obj & gt_j)          int64 [n][G]
 *   gt_area[j]  += #gt_j
 * All counts are exact int64 (zero on entry); pixels whose key lies outside [0, n) only count in gt_area.  The histogram is kept in LDS
 * per workgroup and reaches memory through one atomic per non-zero bin.  1 <= n <= PD_ASSIGN_MAX_KEYS, 0 <= G <= PD_ASSIGN_MAX_GT
 * (gt, inter and gt_area may be null when G == 0), hw > 0.
 */
typedef struct PdAssignHistogram {
  const int16_t *key;
  const uint8_t *obj;
  const uint8_t *gt;
  int64_t *won, *area, *inter, *gt_area;
  int32_t n, G;
  int64_t hw;
} PdAssignHistogram;
int pd_assign_histogram(const PdAssignHistogram *list, int32_t count, void *table_host_pinned, void *table_device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_ASSIGN_H */
