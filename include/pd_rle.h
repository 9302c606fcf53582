/*
 * pd_rle.h — C-ABI of the device COCO run-length codec of libpd_hip.so.
 *
 * Replaces the dense host copies around the reference's pseudo-label files,
 *   utils/utils.py:15-32 (`proposals_to_coco_json` -> pycocotools mask_util.encode of every mask) on the way out and
 *   continuously_postprocess_dcrf.py (mask_util.decode of every mask, `cmask = sum_c mask_c * (c + 1)`) on the way in.
 * The host keeps the ASCII step (run lengths <-> 5-bit groups, utils/rle.py); only run tables cross the bus:
 *
 *   pd_rle_plane_runs    n uint8 planes [H, W] -> the runs of their COLUMN-major flattenings (pos = x * H + y, COCO's order; a run that
 *                        reaches the bottom of column x continues into the top of column x + 1):
 *                          run_start  int32, run_value uint8   all planes back to back, ascending inside a plane, first start 0
 *                          plane_offset int32 [n + 1]          exclusive prefix of the run counts (always complete)
 *                          plane_nonzero int64 [n]             exact number of non-zero pixels
 *                        `binary` != 0: a pixel's value is (byte != 0), reported as 0 / 1; `binary` == 0: the byte itself (label maps —
 *                        runs of two different non-zero labels never merge).  No entry at or beyond `capacity` (in runs) is written;
 *                        plane_offset[n] is the true total also when it exceeds `capacity` (the caller grows its buffers and calls again).
 *                        Three launches: count per (plane, column, segment of PD_RLE_SEG_ROWS rows), exclusive scan in that order,
 *                        boundaries recomputed and written at the scanned offsets.  No atomics, no workgroup waits for another: the table
 *                        is in order and bit-reproducible.
 *   pd_rle_masked_label_runs   exactly pd_rle_plane_runs(..., binary = 0, ...) of the VIRTUAL planes v[p][y][x] = planes[p][y][x] ?
 *                        labels[y][x] : 0, with ONE label map uint8 [H, W] (row-major, contiguous) under all planes: "the labels under
 *                        mask p" (the parts of an object) as run tables without a dense plane per (mask, label) or per
 *                        mask.  plane_nonzero counts v != 0.  The same three launches (the pixel fetch is a template parameter of the
 *                        count / write pass), the same workspace query, the same limits.
 *   pd_rle_decode        run starts -> labels int32 [H, W] (row-major), labels[y][x] = sum over the masks i covering the pixel of (i + 1),
 *                        and / or masks uint8 [n, H, W].  Either output may be null, not both.  Every pixel of every output is written
 *                        (n = 0 with labels: zeros).
 *
 * planes: n planes `plane_stride` BYTES apart, each row-major and contiguous.  starts / offsets: pd_rle_sample_u8's format (pd_input.h):
 * for mask i the entries [offsets[i], offsets[i + 1]) of `starts` are the EXCLUSIVE prefix sums of its COCO run lengths (first run = zeros).
 * workspace: pd_rle_runs_workspace_bytes(n, H, W) bytes of device memory, contents irrelevant before and after (nothing is allocated here).
 * Limits: H * W <= 2^31 - 1; n * H * W <= 2^31 - 1 (run indices are int32); n * ceil(W / 64) * 64 * ceil(H / PD_RLE_SEG_ROWS) <= 2^31 - 1
 * (the workspace-size query returns -1 beyond them).  `stream` = hipStream_t; returns 0 or PD_ERR_*.
 */
#ifndef PD_RLE_H
#define PD_RLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_RLE_SEG_ROWS 8

int pd_rle_seg_rows(void);

int64_t pd_rle_runs_workspace_bytes(int n, int H, int W);

int pd_rle_plane_runs(const uint8_t *planes, int64_t plane_stride, int n, int H, int W, int binary, int capacity, int32_t *run_start,
                      uint8_t *run_value, int32_t *plane_offset, int64_t *plane_nonzero, void *workspace, void *stream);

int pd_rle_masked_label_runs(const uint8_t *planes, int64_t plane_stride, int n, int H, int W, const uint8_t *labels, int capacity,
                             int32_t *run_start, uint8_t *run_value, int32_t *plane_offset, int64_t *plane_nonzero, void *workspace,
                             void *stream);

int pd_rle_decode(const int32_t *starts, const int32_t *offsets, int n, int H, int W, int32_t *labels, uint8_t *masks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_RLE_H */
