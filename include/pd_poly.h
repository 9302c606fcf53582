/*
 * pd_poly.h — C-ABI of the polygon rasteriser of libpd_hip.so.
 *
 * Replaces the per-image CPU work of the reference's PartImageNet mapper (data/dataset_mappers/part_imagenet_mapper.py:
 * convert_coco_poly_to_mask = pycocotools frPyObjects + decode per part, at the OUTPUT resolution, so nothing can be prepared once per
 * image).  The rasteriser is pycocotools' rleFrPoly restated (parity with pycocotools itself is UNPINNED: it is not available to test
 * against): vertices are upsampled by 5 with (int)(5 * x + .5) (C truncation), every edge is walked in unit steps of its longer axis with
 * the other coordinate (int)(start + slope * t + .5) in double arithmetic WITHOUT fused multiply-add, every step that moves from upsampled
 * column 5 * X + 2 to 5 * X + 3 with 0 <= X < w emits the boundary position  a = X * h + clamp(ceil((v - 2) / 5), 0, h)  (v = the smaller
 * upsampled row of the two points; a == (X + 1) * h marks "below the last row"), and pixel p of the column-major flattening is set iff the
 * number of a <= p is odd.
 *
 *   pd_poly_crossings_i32   n polygons in one launch; polygon i has the vertices [vert_offsets[i], vert_offsets[i + 1]) of xy (interleaved
 *                         x, y, float64, ALREADY transformed to the h x w canvas) and fills
 *                         starts[table_offsets[i] .. table_offsets[i + 1]) with 0 followed by its boundary positions in ascending order —
 *                         the run-starts format of pd_input.h: repeated entries are zero-length runs and cancel in the parity, so the
 *                         tables go to pd_rle_sample_groups_u8 (with H = h, W = w) as they are, and a group of several polygons is
 *                         their OR.  The table length of a polygon is 1 + the sum over its edges (x0, x1 = the upsampled columns of
 *                         the edge's ends) of the count of X in [0, w - 1] with min(x0, x1) <= 5 * X + 2 <= max(x0, x1) - 1: the host
 *                         computes table_offsets exactly (partdistillation_amd/functions/polygon.py), there is no count pass and no
 *                         readback.  The kernel never writes outside a polygon's slice whatever the offsets say; a slice longer than
 *                         the polygon needs is padded with 0x7fffffff.
 *                         One workgroup per polygon (grid-stride over polygons).  A table of up to PD_POLY_LDS_ENTRIES boundary positions
 *                         is collected and sorted in LDS and stored with coalesced writes; a longer one is collected and sorted in
 *                         place in global memory by the same launch — no polygon size is refused.
 *                         Upsampled coordinates are clamped to +-(2^30 - 1) (the host refuses |5 x + .5| >= 2^30 before that) and a
 *                         non-finite coordinate counts as 0, so no integer of the walk overflows.  The slopes are exact restatements for
 *                         coordinates up to 2^20 upsampled units (far above PD_CANVAS_MAX_SIDE * 5), where a steep edge's column moves by
 *                         at most one per step.
 *                         PD_ERR_INVALID_ARG before any launch: n < 0, h or w outside 1..PD_CANVAS_MAX_SIDE, h * w > 2^31 - 1, a null
 *                         pointer with n > 0.  n == 0 returns PD_OK without a launch.
 *
 * `stream` = hipStream_t; returns 0 or PD_ERR_*.
 */
#ifndef PD_POLY_H
#define PD_POLY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_POLY_LDS_ENTRIES 4096
int pd_poly_crossings_i32(const double *xy, const int32_t *vert_offsets, int n, int h, int w, const int32_t *table_offsets, int32_t *starts,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_POLY_H */
