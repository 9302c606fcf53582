/*
 * pd_input.h — C-ABI of the device input pipeline of libpd_hip.so.
 *
 * Replaces the per-image CPU work of the reference's dataloader workers,
 *   data/dataset_mappers/proposal_dataset_mapper.py:171-235 (`_forward`, `_transform_annotations`):
 *   T.apply_transform_gens([RandomFlip, RandomCrop, ResizeScale, FixedSizeCrop]) on the image (detectron2 ResizeTransform =
 *   Pillow BILINEAR on uint8), transform_instance_annotations + annotations_to_instances on every pseudo-label
 *   (pycocotools RLE decode -> dense mask -> flip / crop / Pillow NEAREST resize / crop / pad -> BitMasks).
 * The host keeps what is host work: file decode, the random parameter draws, the RLE string -> run lengths parse and the
 * (tiny) Pillow coefficient tables; everything that touches pixels runs here:
 *
 *   pd_resample_rows_u8   horizontal pass of Pillow's 8-bit resample (Resample.c ImagingResampleHorizontal_8bpc):
 *                         tmp[r][x][c] = clip8((2^21 + sum_k src[row0 + r][col(xmin[x] + k)][c] * kk[x][k]) >> 22),
 *                         col(j) = x0 + j, mirrored (W - 1 - col) when `flip` — flip and first crop are just addressing
 *   pd_resample_cols_canvas_u8   vertical pass + second crop + pad (+ HWC -> CHW) onto a RECTANGULAR out_h x out_w canvas:
 *                         y < vh && x < vw ? clip8((2^21 + sum_k tmp[ymin[y] + k - r0][x][c] * kk[y][k]) >> 22) : pad_value,
 *                         planar = 1: out[c][y][x], what the mappers return; planar = 0: out[y][x][c], the HWC layout
 *                         pd_resample_rows_u8 reads, so the base resize of the mappers (ResizeScale(1, 1, base, base)
 *                         [+ FixedSizeCrop((base, base))] ahead of the augmentations) feeds the next resize as it is.  A canvas has at
 *                         least one pixel and sides of at most PD_CANVAS_MAX_SIDE (anything else is PD_ERR_INVALID_ARG, as are
 *                         vh > out_h, vw > out_w, vw > tmp_w, ksize <= 0 and a null pointer that would be read or written), so there is
 *                         no empty request: vh = 0 or vw = 0 launches and fills the canvas with pad_value
 *   pd_rle_sample_u8      all masks of the image, straight from their run lengths (no dense full-resolution mask):
 *                         out[i][y][x] = inside ? parity(search(starts_i, colmajor(src_x[x], src_y[y]))) : 0, and
 *                         area[i] += popcount — src_x / src_y = the composed nearest-neighbour index tables
 *   pd_rle_sample_groups_u8   the ground-truth mappers' sampling (reference voc_parts_mapper.py / cityscapes_part_mapper.py: decode, Pillow
 *                         NEAREST resize, flip, crop, then the per-object, per-class merge): n member masks, n_groups RECTANGULAR output
 *                         planes given as a CSR list of member indices (group g = group_members[group_offsets[g] .. group_offsets[g + 1])),
 *                         out[g][y][x] = OR over the members m of g of parity(search(starts_m, src_x[x] * H + src_y[y]))   (0 / 1),
 *                         member_area[m] = set output pixels of member m on its own (also of a member that is in no group),
 *                         group_area[g]  = set pixels of plane g (the union is counted once).
 *                         src_x[out_w] / src_y[out_h] are source columns / rows in any order, with repeats and gaps: the host composes
 *                         resize, flip and crop into them, so there is no flip argument and no inside window.  A member may be in none,
 *                         one or several groups, a group may be empty (plane and area 0).  out is [n_groups, out_h, out_w] contiguous.
 *                         EVERY byte of out, member_area and group_area is written by the call (the counts are zeroed by the entry point;
 *                         the caller pre-zeroes nothing); the counts are integer sums, so the result is bit-reproducible.
 *                         PD_ERR_INVALID_ARG before any launch: a negative n or n_groups, n_groups > PD_SAMPLE_GROUPS_MAX, H or W < 1,
 *                         H * W > 2^31 - 1, out_h or out_w outside 1..PD_CANVAS_MAX_SIDE, a null pointer that would be read or written
 *                         (group_members may be null when n == 0 or n_groups == 0: it is not read then).  n_groups == 0 still fills
 *                         member_area; n == 0 fills the planes and group_area with zeros; n == 0 && n_groups == 0 returns PD_OK without
 *                         a launch.  The launch is a flat grid-stride one, so no grid dimension grows with n, n_groups or the canvas;
 *                         PD_SAMPLE_GROUPS_MAX only bounds the plane count an image can ask for.  group_members come from the host:
 *                         the caller checks their range (the kernel skips an index outside [0, n) rather than read through it).
 *   pd_rle_sample_groups_canvas_u8   the same sampling onto a PADDED canvas (reference imagenet_part_ranking_dataset_mapper.py: FixedSizeCrop's
 *                         zero pad of the masks, then `gt_masks.tensor.sum(0)[None]`): the contract above with a valid window of vh x vw in the
 *                         top-left corner of each out_h x out_w plane.  src_x has vw entries and src_y has vh;
 *                         out[g][y][x] for y < vh && x < vw is the OR over the group's members as above, every other byte of the plane is 0
 *                         and counts in neither area.  vh == 0 or vw == 0 still writes all-zero planes and zero counts.  The argument
 *                         checks are those above, plus: vh or vw negative, vh > out_h or vw > out_w are PD_ERR_INVALID_ARG (before the
 *                         memsets and the launch); src_x / src_y may be null only when the window is empty.  pd_rle_sample_groups_u8 is
 *                         this entry with vh = out_h, vw = out_w: one kernel serves both.
 *
 * src: uint8 [H, W, 3] (HWC, as decoded).  Tables int32.  kk: Pillow's 22-bit fixed-point coefficients [n, ksize].
 * starts: int32, for mask i the entries [offsets[i], offsets[i+1]) are the EXCLUSIVE prefix sums of its COCO run lengths
 * (column-major, first run = zeros).  `stream` = hipStream_t; returns 0 or PD_ERR_*.
 */
#ifndef PD_INPUT_H
#define PD_INPUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int pd_resample_rows_u8(const uint8_t *src, int H, int W, int row0, int rows, int x0, int flip, const int32_t *xmin,
                        const int32_t *cnt, const int32_t *kk, int ksize, int out_w, uint8_t *tmp, void *stream);

#define PD_CANVAS_MAX_SIDE 65535
int pd_resample_cols_canvas_u8(const uint8_t *tmp, int tmp_rows, int tmp_w, int r0, const int32_t *ymin, const int32_t *cnt,
                               const int32_t *kk, int ksize, int vh, int vw, int out_h, int out_w, int pad_value, int planar,
                               uint8_t *out, void *stream);

int pd_rle_sample_u8(const int32_t *starts, const int32_t *offsets, int n_masks, int H, int W, int flip, const int32_t *src_x,
                     const int32_t *src_y, int vh, int vw, int S, uint8_t *out, int32_t *area, void *stream);

#define PD_SAMPLE_GROUPS_MAX (1 << 20)
int pd_rle_sample_groups_u8(const int32_t *starts, const int32_t *offsets, int n, int H, int W, const int32_t *src_x, const int32_t *src_y,
                            int out_h, int out_w, const int32_t *group_offsets, const int32_t *group_members, int n_groups, uint8_t *out,
                            int32_t *member_area, int32_t *group_area, void *stream);

int pd_rle_sample_groups_canvas_u8(const int32_t *starts, const int32_t *offsets, int n, int H, int W, const int32_t *src_x, const int32_t *src_y,
                                   int vh, int vw, int out_h, int out_w, const int32_t *group_offsets, const int32_t *group_members,
                                   int n_groups, uint8_t *out, int32_t *member_area, int32_t *group_area, void *stream);

/*
 * out [B, H, W, 3] fp32 (the channels-last storage of the [B, 3, H, W] batch) = (images[b] - mean) / std for B same-size planar uint8
 * images [3, H, W] — the model's preprocess (reference proposal_model.py:251-253 / part_distillation_model.py: `(x - pixel_mean) /
 * pixel_std` per image) in one launch.  images: HOST array of B device pointers; mean3 / std3: HOST arrays of 3 floats.
 */
#define PD_NORMALIZE_MAX_IMAGES 16
int pd_normalize_u8_nhwc(const uint8_t *const *images, int B, int H, int W, const float *mean3, const float *std3, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_INPUT_H */
