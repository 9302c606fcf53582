/*
 * pd_eval.h — C-ABI of the evaluation counters of libpd_hip.so (csrc/evaluation.hip): proposal AR@k and part mIoU.
 *
 * What it replaces: the reference's evaluators copy every predicted and ground-truth mask to the host in full resolution, RLE-encode
 * them (pycocotools) and paint label maps one torch.where per mask before np.bincount (part_distillation/evaluation/
 * proposal_evaluator.py, miou_evaluator.py, miou_matcher.py).  The metrics only need integer counts; these kernels produce them on the
 * device from bit planes, and only a few hundred bytes of counters per image reach the host.
 *
 * Every count is an exact integer (int64 atomics, no floating-point accumulation): results are deterministic.
 * A batch of images is ONE launch per kernel: the caller passes a host list of descriptors, a pinned staging buffer and a device
 * buffer of pd_eval_table_bytes(count) bytes each (the pinned one must stay untouched until the asynchronous copy has executed).
 * All other pointers are device pointers; `stream` = hipStream_t; returns 0 or PD_ERR_* (pd_msda.h) with pd_last_error() set.
 */
#ifndef PD_EVAL_H
#define PD_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_EVAL_LIMITS 5              /* AR@1, 10, 50, 100, 200 */
#define PD_EVAL_THRESHOLDS 10         /* IoU 0.50 : 0.05 : 0.95 */
#define PD_EVAL_MAX_ROWS 200          /* largest AR limit: rows of the IoU matrix the greedy cover reads */
#define PD_EVAL_MAX_GT 64             /* ground-truth masks per image */
#define PD_EVAL_LDS_BINS 8192         /* confusion tables with (n + 1)^2 <= this are histogrammed in LDS, larger ones with global atomics */

int64_t pd_eval_table_bytes(int32_t count);

/* Bit planes: masks [n][hw] (bool / uint8, non-zero = set, contiguous) -> bits [n][words] (words = ceil(hw / 64); pixel q of a mask is
 * bit q % 64 of word q / 64, bits past hw are 0) and area[i] += number of set pixels (area zero on entry).  Reads the masks once. */
typedef struct PdEvalMaskSet {
  const uint8_t *masks;
  uint64_t *bits;
  int64_t *area;
  int32_t n;
  int32_t reserved;
  int64_t hw;
} PdEvalMaskSet;
int pd_eval_pack_grouped(const PdEvalMaskSet *list, int32_t count, void *table_host_pinned, void *table_device, void *stream);

/* Pairwise intersections: inter[r][j] += popcount(a[rows[r]] & b[j]) over all words, r < p, j < g (inter zero on entry).
 * rows: nullable int64 [p] (row r of the result is plane r of a when null).  p >= 1, 1 <= g <= PD_EVAL_MAX_GT. */
typedef struct PdEvalPairs {
  const uint64_t *a;
  const int64_t *rows;
  const uint64_t *b;
  int64_t *inter;
  int32_t p, g;
  int64_t words;
} PdEvalPairs;
int pd_eval_intersect_grouped(const PdEvalPairs *list, int32_t count, void *table_host_pinned, void *table_device, void *stream);

/* Label maps and confusion table: every pixel's predicted label is the class of the LAST pred mask covering it (n when none), its
 * ground-truth label likewise from the gt masks; conf[slot][pd][gt] += 1 with conf int64 [num_slots][n + 1][n + 1] and slot = *slot (a
 * device int64, the image's object class).  Images whose slot lies outside [0, num_slots) and pixels whose label lies outside [0, n]
 * are not counted.  pred_n, gt_n >= 0. */
typedef struct PdEvalConfusion {
  const uint64_t *pred_bits;          /* [pred_n][words] */
  const int64_t *pred_cls;            /* [pred_n] */
  const uint64_t *gt_bits;            /* [gt_n][words] */
  const int64_t *gt_cls;              /* [gt_n] */
  const int64_t *slot;
  int32_t pred_n, gt_n;
  int64_t hw;
} PdEvalConfusion;
int pd_eval_confusion_grouped(const PdEvalConfusion *list, int32_t count, int32_t n, int64_t *conf, int32_t num_slots,
                              void *table_host_pinned, void *table_device, void *stream);

/* Greedy cover of the box-proposal recall (one workgroup per image).  The IoU matrix is inter[r][j] / (area_p[rows[r]] + area_g[j] -
 * inter[r][j]) in float64 (0 when the union is 0) over the proposals in score order (rows r < p <= PD_EVAL_MAX_ROWS; rows nullable as
 * above) and the gts with 0 < area_g <= 1e10 (in their order; g <= PD_EVAL_MAX_GT before the filter).  For every limit L of
 * {1, 10, 50, 100, 200}, min(min(p, L), kept gts) rounds on the first min(p, L) rows: column maxima (first row on ties), their maximum
 * (first column on ties), record it, retire its row and column.  Each recorded value is rounded to float32 and compared with the float32
 * thresholds[PD_EVAL_THRESHOLDS]: hits[L][t] += #(value >= thresholds[t]); num_pos[L] += kept gts. */
typedef struct PdEvalRecall {
  const int64_t *inter;               /* [p][g] */
  const int64_t *rows;
  const int64_t *area_p, *area_g;
  int32_t p, g;
} PdEvalRecall;
int pd_eval_recall_grouped(const PdEvalRecall *list, int32_t count, const float *thresholds, int64_t *hits, int64_t *num_pos,
                           void *table_host_pinned, void *table_device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_EVAL_H */
