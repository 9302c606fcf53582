// Device input pipeline (include/pd_input.h): Pillow-exact 8-bit bilinear resample in two passes with flip / crops / pad
// folded into the addressing (onto the square training canvas, or a rectangular base canvas), and mask sampling straight from COCO run
// lengths.  All of these kernels are byte streams
// (HBM-bound at a few MB per image); the point is to take ~10 ms of per-image CPU work off the dataloader.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_input.h"
#include "pd_msda.h"

namespace {
constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ uint8_t clip8(int v)
{
  v >>= PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one thread per (row, output column): 3 channels, taps contiguous in the source row
__global__ __launch_bounds__(256) void resample_rows(const uint8_t *__restrict__ src, int W, int row0, int rows, int x0, int flip,
                                                     const int32_t *__restrict__ xmin, const int32_t *__restrict__ cnt,
                                                     const int32_t *__restrict__ kk, int ksize, int out_w, uint8_t *__restrict__ tmp)
{
  const int x = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (x >= out_w) return;
  const uint8_t *row = src + (int64_t)(row0 + r) * W * 3;
  const int32_t *k = kk + (int64_t)x * ksize;
  const int first = x0 + xmin[x], n = cnt[x];
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int j = 0; j < n; ++j) {
    const int col = flip ? W - 1 - (first + j) : first + j;
    const uint8_t *p = row + col * 3;
    const int w = k[j];
    a0 += p[0] * w; a1 += p[1] * w; a2 += p[2] * w;
  }
  uint8_t *o = tmp + ((int64_t)r * out_w + x) * 3;
  o[0] = clip8(a0); o[1] = clip8(a1); o[2] = clip8(a2);
}

// one thread per output pixel of the out_h x out_w canvas, all 3 channel planes
__global__ __launch_bounds__(256) void resample_cols(const uint8_t *__restrict__ tmp, int tmp_w, int r0, const int32_t *__restrict__ ymin,
                                                     const int32_t *__restrict__ cnt, const int32_t *__restrict__ kk, int ksize, int vh,
                                                     int vw, int out_h, int out_w, int pad_value, uint8_t *__restrict__ out)
{
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= out_w) return;
  int a0, a1, a2;
  if (y < vh && x < vw) {
    const int32_t *k = kk + (int64_t)y * ksize;
    const int first = ymin[y] - r0, n = cnt[y];
    a0 = a1 = a2 = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < n; ++j) {
      const uint8_t *p = tmp + ((int64_t)(first + j) * tmp_w + x) * 3;
      const int w = k[j];
      a0 += p[0] * w; a1 += p[1] * w; a2 += p[2] * w;
    }
    a0 = clip8(a0); a1 = clip8(a1); a2 = clip8(a2);
  } else {
    a0 = a1 = a2 = pad_value;
  }
  const int64_t plane = (int64_t)out_h * out_w, o = (int64_t)y * out_w + x;
  out[o] = (uint8_t)a0; out[plane + o] = (uint8_t)a1; out[2 * plane + o] = (uint8_t)a2;
}

// the same pass onto an interleaved [out_h, out_w, 3] canvas, one thread per BYTE of a canvas row: a tmp row has the same pixel-major,
// channel-minor order, so byte e of the row is tapped at byte e of the tmp rows — every tap is 64 consecutive bytes per wave, and so is the store
__global__ __launch_bounds__(256) void resample_cols_hwc(const uint8_t *__restrict__ tmp, int tmp_w, int r0, const int32_t *__restrict__ ymin,
                                                         const int32_t *__restrict__ cnt, const int32_t *__restrict__ kk, int ksize, int vh,
                                                         int vw, int out_w, int pad_value, uint8_t *__restrict__ out)
{
  const int e = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (e >= out_w * 3) return;
  int a = pad_value;
  if (y < vh && e < vw * 3) {
    const int32_t *k = kk + (int64_t)y * ksize;
    const int first = ymin[y] - r0, n = cnt[y];
    a = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < n; ++j) a += tmp[(int64_t)(first + j) * tmp_w * 3 + e] * k[j];
    a = clip8(a);
  }
  out[(int64_t)y * out_w * 3 + e] = (uint8_t)a;
}

// one thread per (mask, output pixel): binary search of the pixel's column-major position in the mask's run starts
__global__ __launch_bounds__(256) void rle_sample(const int32_t *__restrict__ starts, const int32_t *__restrict__ offsets, int H, int W,
                                                  int flip, const int32_t *__restrict__ src_x, const int32_t *__restrict__ src_y, int vh,
                                                  int vw, int S, uint8_t *__restrict__ out, int32_t *__restrict__ area)
{
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, i = blockIdx.z;
  int v = 0;
  if (x < S && y < vh && x < vw) {
    const int sx = flip ? W - 1 - src_x[x] : src_x[x];
    const int pos = sx * H + src_y[y];
    v = pd_rle_find_run(starts + offsets[i], offsets[i + 1] - offsets[i], pos) & 1;
  }
  if (x < S) out[((int64_t)i * S + y) * S + x] = (uint8_t)v;
  const unsigned long long ball = __ballot(v != 0);
  if ((threadIdx.x & 63) == 0 && ball) atomicAdd(area + i, __popcll(ball));
}
// pd_rle_sample_groups_u8 / pd_rle_sample_groups_canvas_u8: one work unit per output plane (the OR of a group's members) and one per member
// (its own pixel count), cut into tiles of SG_TILE consecutive pixels of the flat out_h x out_w plane, so every store is 64 consecutive
// bytes per wave whatever the pitch.
// A thread keeps the column-major positions of its SG_PIX pixels in registers; the members of the unit pass through LDS one after the
// other (a run table is a few hundred bytes and is searched 2048 times per tile), tables longer than SG_LDS_RUNS are searched in place.
// Only the vh x vw window in the top-left corner of a plane is sampled (the whole plane for pd_rle_sample_groups_u8): a pixel outside it
// reads no table and is a 0 that counts in no area.
constexpr int SG_PIX = 8, SG_TILE = 256 * SG_PIX, SG_LDS_RUNS = 2048, SG_MAX_BLOCKS = 4096;

__global__ __launch_bounds__(256) void rle_sample_groups(const int32_t *__restrict__ starts, const int32_t *__restrict__ offsets, int n, int H,
                                                         const int32_t *__restrict__ src_x, const int32_t *__restrict__ src_y, uint32_t vh,
                                                         uint32_t vw, uint32_t out_w, uint32_t plane, const int32_t *__restrict__ group_offsets,
                                                         const int32_t *__restrict__ group_members, int n_groups, uint8_t *__restrict__ out,
                                                         int32_t *__restrict__ member_area, int32_t *__restrict__ group_area,
                                                         uint32_t tiles_per_plane, int64_t total_tiles)
{
  __shared__ int32_t runs[SG_LDS_RUNS];
  __shared__ int tile_count;
  const int tid = threadIdx.x;
  for (int64_t t = blockIdx.x; t < total_tiles; t += gridDim.x) {
    const int unit = (int)(t / tiles_per_plane);
    const uint32_t p0 = (uint32_t)(t - (int64_t)unit * tiles_per_plane) * SG_TILE + tid;
    int pos[SG_PIX];
#pragma unroll
    for (int k = 0; k < SG_PIX; ++k) {
      const uint32_t p = p0 + k * 256;
      pos[k] = -1;                                                        // past the plane or the window: before every run start, value 0
      if (p < plane) {
        const uint32_t y = p / out_w, x = p - y * out_w;
        if (y < vh && x < vw) pos[k] = src_x[x] * H + src_y[y];
      }
    }
    const bool is_group = unit < n_groups;
    int mb = unit - n_groups, me = mb + 1;                                // a member on its own
    if (is_group) { mb = group_offsets[unit]; me = n > 0 ? group_offsets[unit + 1] : mb; }
    if (tid == 0) tile_count = 0;
    unsigned bits = 0;
    for (int j = mb; j < me; ++j) {                                       // block-uniform: the barriers below are reached by all
      const int m = is_group ? group_members[j] : j;
      if ((unsigned)m >= (unsigned)n) continue;
      const int a = offsets[m], cnt = offsets[m + 1] - a;
      if (cnt <= SG_LDS_RUNS) {
        __syncthreads();                                                  // the searches of the member before
        for (int i = tid; i < cnt; i += 256) runs[i] = starts[a + i];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SG_PIX; ++k)
          if (!((bits >> k) & 1)) bits |= (unsigned)(pd_rle_find_run(runs, cnt, pos[k]) & 1) << k;
      } else {
#pragma unroll
        for (int k = 0; k < SG_PIX; ++k)
          if (!((bits >> k) & 1)) bits |= (unsigned)(pd_rle_find_run(starts + a, cnt, pos[k]) & 1) << k;
      }
    }
    if (is_group) {
      uint8_t *o = out + (int64_t)unit * plane;
#pragma unroll
      for (int k = 0; k < SG_PIX; ++k) {
        const uint32_t p = p0 + k * 256;
        if (p < plane) o[p] = (uint8_t)((bits >> k) & 1);
      }
    }
    // counts: wave, then block through LDS, then one global atomic per tile, zeros skipped
    int c = __popc(bits);
#pragma unroll
    for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off);
    __syncthreads();                                                      // tile_count = 0 is visible
    if ((tid & 63) == 0 && c) atomicAdd(&tile_count, c);
    __syncthreads();
    if (tid == 0 && tile_count) atomicAdd(is_group ? group_area + unit : member_area + (unit - n_groups), tile_count);
  }
}
}  // namespace

extern "C" int pd_resample_rows_u8(const uint8_t *src, int H, int W, int row0, int rows, int x0, int flip, const int32_t *xmin,
                                   const int32_t *cnt, const int32_t *kk, int ksize, int out_w, uint8_t *tmp, void *stream_)
{
  if (H <= 0 || W <= 0 || rows < 0 || out_w < 0 || row0 < 0 || row0 + rows > H || ksize <= 0)
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_resample_rows_u8: bad sizes H=%d W=%d row0=%d rows=%d out_w=%d", H, W, row0, rows, out_w);
  if (rows == 0 || out_w == 0) return PD_OK;
  if (!src || !xmin || !cnt || !kk || !tmp) return pd_set_error(PD_ERR_INVALID_ARG, "pd_resample_rows_u8: null pointer");
  hipLaunchKernelGGL(resample_rows, dim3((out_w + 255) / 256, rows), dim3(256), 0, (hipStream_t)stream_, src, W, row0, rows, x0, flip,
                     xmin, cnt, kk, ksize, out_w, tmp);
  return pd_check_launch("pd_resample_rows_u8");
}

extern "C" int pd_resample_cols_canvas_u8(const uint8_t *tmp, int tmp_rows, int tmp_w, int r0, const int32_t *ymin, const int32_t *cnt,
                                          const int32_t *kk, int ksize, int vh, int vw, int out_h, int out_w, int pad_value, int planar,
                                          uint8_t *out, void *stream_)
{
  if (out_h <= 0 || out_w <= 0 || out_h > PD_CANVAS_MAX_SIDE || out_w > PD_CANVAS_MAX_SIDE || vh < 0 || vw < 0 || vh > out_h || vw > out_w ||
      vw > tmp_w || ksize <= 0)
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_resample_cols_canvas_u8: bad sizes canvas=%dx%d (sides 1..%d) vh=%d vw=%d tmp_w=%d ksize=%d", out_h,
                        out_w, PD_CANVAS_MAX_SIDE, vh, vw, tmp_w, ksize);
  if (!out || (vh > 0 && vw > 0 && (!tmp || !ymin || !cnt || !kk)))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_resample_cols_canvas_u8: null pointer");
  if (planar)
    hipLaunchKernelGGL(resample_cols, dim3((out_w + 255) / 256, out_h), dim3(256), 0, (hipStream_t)stream_, tmp, tmp_w, r0, ymin, cnt, kk,
                       ksize, vh, vw, out_h, out_w, pad_value, out);
  else
    hipLaunchKernelGGL(resample_cols_hwc, dim3((out_w * 3 + 255) / 256, out_h), dim3(256), 0, (hipStream_t)stream_, tmp, tmp_w, r0, ymin, cnt,
                       kk, ksize, vh, vw, out_w, pad_value, out);
  return pd_check_launch("pd_resample_cols_canvas_u8");
}

extern "C" int pd_rle_sample_u8(const int32_t *starts, const int32_t *offsets, int n_masks, int H, int W, int flip, const int32_t *src_x,
                                const int32_t *src_y, int vh, int vw, int S, uint8_t *out, int32_t *area, void *stream_)
{
  if (n_masks < 0 || S <= 0 || H <= 0 || W <= 0 || vh < 0 || vw < 0 || vh > S || vw > S || (int64_t)H * W > 0x7fffffffLL)
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_rle_sample_u8: bad sizes n=%d S=%d H=%d W=%d", n_masks, S, H, W);
  if (n_masks == 0) return PD_OK;
  if (!starts || !offsets || !out || !area || (vh > 0 && vw > 0 && (!src_x || !src_y)))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_rle_sample_u8: null pointer");
  hipLaunchKernelGGL(rle_sample, dim3((S + 255) / 256, S, n_masks), dim3(256), 0, (hipStream_t)stream_, starts, offsets, H, W, flip, src_x,
                     src_y, vh, vw, S, out, area);
  return pd_check_launch("pd_rle_sample_u8");
}

namespace {
// the shared tail of the two sampling entry points, after their argument checks
int launch_sample_groups(const char *who, const int32_t *starts, const int32_t *offsets, int n, int H, const int32_t *src_x, const int32_t *src_y,
                         int vh, int vw, int out_h, int out_w, const int32_t *group_offsets, const int32_t *group_members, int n_groups,
                         uint8_t *out, int32_t *member_area, int32_t *group_area, hipStream_t stream)
{
  // the counts are atomic sums: zero them here, the caller pre-zeroes nothing (the planes are written whole by the kernel)
  if (n > 0 && hipMemsetAsync(member_area, 0, (size_t)n * sizeof(int32_t), stream) != hipSuccess) return pd_check_launch(who);
  if (n_groups > 0 && hipMemsetAsync(group_area, 0, (size_t)n_groups * sizeof(int32_t), stream) != hipSuccess) return pd_check_launch(who);
  const uint32_t plane = (uint32_t)out_h * (uint32_t)out_w;               // <= 65535^2 < 2^32
  const uint32_t tiles_per_plane = (plane + SG_TILE - 1) / SG_TILE;
  const int64_t total = ((int64_t)n_groups + n) * tiles_per_plane;
  // a flat grid-stride launch: no grid dimension grows with the planes, the members or the canvas
  const unsigned grid = (unsigned)(total < SG_MAX_BLOCKS ? total : SG_MAX_BLOCKS);
  hipLaunchKernelGGL(rle_sample_groups, dim3(grid), dim3(256), 0, stream, starts, offsets, n, H, src_x, src_y, (uint32_t)vh, (uint32_t)vw,
                     (uint32_t)out_w, plane, group_offsets, group_members, n_groups, out, member_area, group_area, tiles_per_plane, total);
  return pd_check_launch(who);
}
}  // namespace

extern "C" int pd_rle_sample_groups_u8(const int32_t *starts, const int32_t *offsets, int n, int H, int W, const int32_t *src_x,
                                       const int32_t *src_y, int out_h, int out_w, const int32_t *group_offsets, const int32_t *group_members,
                                       int n_groups, uint8_t *out, int32_t *member_area, int32_t *group_area, void *stream_)
{
  if (n < 0 || n_groups < 0 || n_groups > PD_SAMPLE_GROUPS_MAX || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffLL || out_h <= 0 || out_w <= 0 ||
      out_h > PD_CANVAS_MAX_SIDE || out_w > PD_CANVAS_MAX_SIDE)
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_rle_sample_groups_u8: bad sizes n=%d n_groups=%d (<= %d) H=%d W=%d out=%dx%d (sides 1..%d)", n,
                        n_groups, PD_SAMPLE_GROUPS_MAX, H, W, out_h, out_w, PD_CANVAS_MAX_SIDE);
  if (n == 0 && n_groups == 0) return PD_OK;
  if (!src_x || !src_y || (n > 0 && (!starts || !offsets || !member_area)) || (n_groups > 0 && (!group_offsets || !out || !group_area)) ||
      (n > 0 && n_groups > 0 && !group_members))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_rle_sample_groups_u8: null pointer");
  return launch_sample_groups("pd_rle_sample_groups_u8", starts, offsets, n, H, src_x, src_y, out_h, out_w, out_h, out_w, group_offsets,
                              group_members, n_groups, out, member_area, group_area, (hipStream_t)stream_);
}

extern "C" int pd_rle_sample_groups_canvas_u8(const int32_t *starts, const int32_t *offsets, int n, int H, int W, const int32_t *src_x,
                                              const int32_t *src_y, int vh, int vw, int out_h, int out_w, const int32_t *group_offsets,
                                              const int32_t *group_members, int n_groups, uint8_t *out, int32_t *member_area,
                                              int32_t *group_area, void *stream_)
{
  if (n < 0 || n_groups < 0 || n_groups > PD_SAMPLE_GROUPS_MAX || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffffLL || out_h <= 0 || out_w <= 0 ||
      out_h > PD_CANVAS_MAX_SIDE || out_w > PD_CANVAS_MAX_SIDE || vh < 0 || vw < 0 || vh > out_h || vw > out_w)
    return pd_set_error(PD_ERR_INVALID_ARG,
                        "pd_rle_sample_groups_canvas_u8: bad sizes n=%d n_groups=%d (<= %d) H=%d W=%d window=%dx%d canvas=%dx%d (sides 1..%d)", n,
                        n_groups, PD_SAMPLE_GROUPS_MAX, H, W, vh, vw, out_h, out_w, PD_CANVAS_MAX_SIDE);
  if (n == 0 && n_groups == 0) return PD_OK;
  if ((vh > 0 && vw > 0 && (!src_x || !src_y)) || (n > 0 && (!starts || !offsets || !member_area)) ||
      (n_groups > 0 && (!group_offsets || !out || !group_area)) || (n > 0 && n_groups > 0 && !group_members))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_rle_sample_groups_canvas_u8: null pointer");
  return launch_sample_groups("pd_rle_sample_groups_canvas_u8", starts, offsets, n, H, src_x, src_y, vh, vw, out_h, out_w, group_offsets,
                              group_members, n_groups, out, member_area, group_area, (hipStream_t)stream_);
}

// (x - mean) / std of B same-size planar uint8 images [3, H, W] written straight into the channels-last fp32 batch the backbone reads
// (reference proposal_model.py / part_distillation_model.py: `(x - self.pixel_mean) / self.pixel_std` per image, then ImageList.from_tensors)
// — one launch for the batch (was a subtraction per image plus a division over the batch).  The same two fp32 operations per value.
namespace {
struct NormImages { const uint8_t *img[PD_NORMALIZE_MAX_IMAGES]; float mean[3], std[3]; };

__global__ __launch_bounds__(256) void normalize_u8_nhwc(NormImages in, float *__restrict__ out, int B, int64_t hw)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)B * hw; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / hw);
    const int64_t px = i - (int64_t)b * hw;
    const uint8_t *p = in.img[b];
    const float r = ((float)p[px] - in.mean[0]) / in.std[0];
    const float g = ((float)p[hw + px] - in.mean[1]) / in.std[1];
    const float bl = ((float)p[2 * hw + px] - in.mean[2]) / in.std[2];
    float *o = out + i * 3;
    o[0] = r; o[1] = g; o[2] = bl;
  }
}
}  // namespace

extern "C" int pd_normalize_u8_nhwc(const uint8_t *const *images, int B, int H, int W, const float *mean3, const float *std3, float *out, void *stream_)
{
  if (B < 0 || B > PD_NORMALIZE_MAX_IMAGES || H <= 0 || W <= 0) return pd_set_error(PD_ERR_INVALID_ARG, "pd_normalize_u8_nhwc: B=%d (<= %d) H=%d W=%d", B, PD_NORMALIZE_MAX_IMAGES, H, W);
  if (B == 0) return PD_OK;
  if (!images || !mean3 || !std3 || !out) return pd_set_error(PD_ERR_INVALID_ARG, "pd_normalize_u8_nhwc: null pointer");
  NormImages in;
  for (int b = 0; b < B; ++b) {
    if (!images[b]) return pd_set_error(PD_ERR_INVALID_ARG, "pd_normalize_u8_nhwc: null image %d", b);
    in.img[b] = images[b];
  }
  for (int c = 0; c < 3; ++c) { in.mean[c] = mean3[c]; in.std[c] = std3[c]; }
  const int64_t hw = (int64_t)H * W, total = (int64_t)B * hw;
  const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(normalize_u8_nhwc, dim3(grid), dim3(256), 0, (hipStream_t)stream_, in, out, B, hw);
  return pd_check_launch("pd_normalize_u8_nhwc");
}
