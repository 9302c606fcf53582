// Pixel grouping at evaluation (C-ABI in include/pd_grouping.h): the label map and the boolean masks of images whose output size differs
// from the size the network saw.  Both kernels serve a batch of images in one launch through a device table of entries, each with the
// index of its first workgroup (wg_begin, ascending); a workgroup finds its entry by a scan of the (short) table.
//
// A lane owns 4 consecutive pixels of one output row (one 4-byte store, 256 B per wavefront).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_grouping.h"
#include "grouped_table.h"
#include "resize_taps.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kPx = 4;                       // pixels per lane
constexpr int kTileW = 64 * kPx;             // columns per workgroup
constexpr int kMixFloats = 1024;             // row-mixed scores a wavefront keeps in LDS: K * (low-resolution columns under its 256 pixels)
constexpr int kResizeRows = 4;               // rows per wavefront of masks_resize

// ------------------------------------------------------------------------------------------------------------------- label map
// One wavefront per output row segment of 256 pixels.  The row's 4 low-resolution rows are mixed once per (k, low column) into LDS
// (the columns under 256 output pixels: ~19 at the 16x upscale of config 4), then a pixel reads 4 values per k.  A segment whose
// column span does not fit (strong down-scaling) mixes the rows per pixel from global memory instead.  Segments without an object
// pixel only write zeros.
struct LabelsEntry {
  const float *scores;
  const uint8_t *mask;
  uint8_t *labels;
  int32_t *counts;
  int32_t K, h, w, Hi, Wi, H, W, tiles_x;
  float sh1, sw1, sh2, sw2;
  int64_t wg_begin;
};

__global__ void __launch_bounds__(kThreads) scores_argmax_resized(const LabelsEntry *table, int count)
{
  __shared__ float mix_s[kWaves][kMixFloats];
  __shared__ int cnt[PD_GROUPING_MAX_K + 1];
  const LabelsEntry *e = find_entry(table, count, blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = e->K, h = e->h, w = e->w, H = e->H, W = e->W;
  for (int i = tid; i <= K; i += kThreads) cnt[i] = 0;
  const int64_t local = blockIdx.x - e->wg_begin;
  const int tx = (int)(local % e->tiles_x), ty = (int)(local / e->tiles_x);
  const int y = ty * kWaves + wave, xs = tx * kTileW, x0 = xs + lane * kPx;
  const bool row_ok = y < H;
  // (table pointers are made global in uniform control flow: pd_as_global pins them in scalar registers)
  const float *scores = pd_as_global(e->scores);
  const uint8_t *mask = pd_as_global(e->mask);
  uint8_t *labels = pd_as_global(e->labels);
  int32_t *counts = pd_as_global(e->counts);
  const int64_t o = (int64_t)y * W + x0;

  uint8_t m[kPx] = {0, 0, 0, 0};
  bool in[kPx];
#pragma unroll
  for (int j = 0; j < kPx; ++j) in[j] = row_ok && x0 + j < W;
  if (in[0]) load4_u8(mask + o, in[kPx - 1] && aligned4(mask + o), in, m);
  const bool any = __ballot((m[0] | m[1] | m[2] | m[3]) != 0) != 0;          // wave-uniform: this segment has object pixels

  Tap4 ry;
  int cmin = 0, ncols = 0;
  bool use_lds = false;
  float *mix = mix_s[wave];
  auto rowmix = [&](int k, int c) {
    const float *s = scores + (int64_t)k * h * w + c;
    return mix4(ry, [&](int i) { return s[i * w]; });
  };
  if (any) {
    ry = chain_of(y, e->sh2, e->Hi, e->sh1, h);
    const int xe = (xs + kTileW < W ? xs + kTileW : W) - 1;
    // the taps are non-decreasing in the output index (resize_taps.h): first tap of the first pixel, last of the last
    cmin = chain_of(xs, e->sw2, e->Wi, e->sw1, w).i[0];
    ncols = chain_of(xe, e->sw2, e->Wi, e->sw1, w).i[3] - cmin + 1;
    use_lds = ncols * K <= kMixFloats;
    if (use_lds)
      for (int idx = lane; idx < ncols * K; idx += 64) {
        const int k = idx / ncols, c = idx - k * ncols;
        mix[idx] = rowmix(k, cmin + c);
      }
  }
  __syncthreads();

  uint8_t lab[kPx];
#pragma unroll
  for (int j = 0; j < kPx; ++j) lab[j] = in[j] ? 0 : 255;                    // 255: outside the image, counted nowhere
  if (any) {
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
      if (!in[j] || !m[j]) continue;
      const Tap4 cx = chain_of(x0 + j, e->sw2, e->Wi, e->sw1, w);
      float best = -INFINITY;
      int arg = 0;
      for (int k = 0; k < K; ++k) {
        float v;
        if (use_lds) {
          const int b = k * ncols - cmin;
          v = mix4(cx, [&](int i) { return mix[b + i]; });
        } else {
          v = mix4(cx, [&rowmix, k](int i) { return rowmix(k, i); });
        }
        if (v > best) {
          best = v;
          arg = k;
        }
      }
      lab[j] = (uint8_t)(arg + 1);
    }
  }
  if (in[0]) store4_u8(labels + o, in[kPx - 1] && aligned4(labels + o), in, pack4_u8(lab));
  // label counts: per wavefront by ballot, per workgroup in LDS, one global atomic per label present
  for (int l = 0; l <= K; ++l) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < kPx; ++j) c += __popcll(__ballot(lab[j] == l));
    if (lane == 0 && c) atomicAdd(&cnt[l], c);
  }
  __syncthreads();
  for (int l = tid; l <= K; l += kThreads)
    if (cnt[l]) atomicAdd(counts + l, cnt[l]);
}

// ------------------------------------------------------------------------------------------------------------------- mask resize
// A workgroup owns 16 rows x 256 columns of one mask; a lane keeps the column taps of its 4 pixels in registers and walks 4 rows.
struct ResizeEntry {
  const uint8_t *src;
  uint8_t *dst;
  int64_t *area;
  int32_t n, Hp, Wp, Hi, Wi, H, W, tiles_x, tiles_y, pad;
  float sh, sw;
  int64_t wg_begin;
};

__global__ void __launch_bounds__(kThreads) masks_resize(const ResizeEntry *table, int count)
{
  __shared__ uint32_t red[kWaves];
  const ResizeEntry *e = find_entry(table, count, blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = e->H, W = e->W, Wp = e->Wp;
  const int64_t local = blockIdx.x - e->wg_begin;
  const int tx = (int)(local % e->tiles_x);
  const int64_t t = local / e->tiles_x;
  const int ty = (int)(t % e->tiles_y);
  const int64_t i = t / e->tiles_y;
  const uint8_t *src = pd_as_global(e->src) + i * (int64_t)e->Hp * Wp;
  uint8_t *dst = pd_as_global(e->dst) + i * (int64_t)H * W;
  int64_t *area = pd_as_global(e->area);
  const int x0 = tx * kTileW + lane * kPx;
  int c0[kPx], c1[kPx];                                                      // c1 < 0: the second tap has weight 0
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    const Tap tp = tap_of(x0 + j < W ? x0 + j : W - 1, e->sw, e->Wi);
    c0[j] = tp.i0;
    c1[j] = tp.l1 != 0.f ? tp.i1 : -1;
  }
  uint32_t cnt = 0;
  for (int r = 0; r < kResizeRows; ++r) {
    const int y = (ty * kWaves + wave) * kResizeRows + r;
    if (y >= H) break;                                                       // wave-uniform
    const Tap tp = tap_of(y, e->sh, e->Hi);
    const uint8_t *p0 = src + (int64_t)tp.i0 * Wp;
    const uint8_t *p1 = src + (int64_t)tp.i1 * Wp;
    const bool second = tp.l1 != 0.f;
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
      if (x0 + j >= W) continue;
      uint32_t v = p0[c0[j]];
      if (c1[j] >= 0) v |= p0[c1[j]];
      if (second) {
        v |= p1[c0[j]];
        if (c1[j] >= 0) v |= p1[c1[j]];
      }
      out |= (uint32_t)(v != 0) << (8 * j);
    }
    cnt += __popc(out);
    if (x0 < W) {
      uint8_t *dp = dst + (int64_t)y * W + x0;
      if (x0 + kPx <= W && aligned4(dp)) {
        *reinterpret_cast<uint32_t *>(dp) = out;
      } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j)
          if (x0 + j < W) dp[j] = (uint8_t)(out >> (8 * j));
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) red[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    const uint32_t s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(reinterpret_cast<unsigned long long *>(area + i), (unsigned long long)s);
  }
}

bool sizes_ok(int Hp, int Wp, int Hi, int Wi, int H, int W)
{
  return Hp > 0 && Wp > 0 && Hi > 0 && Wi > 0 && Hi <= Hp && Wi <= Wp && H > 0 && W > 0;
}

}  // namespace

extern "C" int64_t pd_grouping_table_bytes(int32_t count)
{
  const size_t m = sizeof(LabelsEntry) > sizeof(ResizeEntry) ? sizeof(LabelsEntry) : sizeof(ResizeEntry);
  return (int64_t)(count > 0 ? count : 0) * (int64_t)m;
}

extern "C" int pd_scores_argmax_resized_u8(const PdGroupLabels *list, int32_t count, void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<LabelsEntry>(
      "pd_scores_argmax_resized_u8", list, count, true, table_host_pinned, table_device, st,
      [](const PdGroupLabels &d, int i, LabelsEntry &e, int64_t wg_begin) -> int64_t {
        if (d.K < 1 || d.K > PD_GROUPING_MAX_K || d.h <= 0 || d.w <= 0 || !sizes_ok(d.Hp, d.Wp, d.Hi, d.Wi, d.H, d.W) ||
            (int64_t)d.K * d.h * d.w >= INT32_MAX || !d.scores || !d.mask || !d.labels || !d.counts)
          return pd_set_error(PD_ERR_INVALID_ARG,
                              "pd_scores_argmax_resized_u8: image %d: K=%d h=%d w=%d Hp=%d Wp=%d Hi=%d Wi=%d H=%d W=%d (1 <= K <= %d, Hi <= Hp, "
                              "Wi <= Wp, non-null pointers required)",
                              i, d.K, d.h, d.w, d.Hp, d.Wp, d.Hi, d.Wi, d.H, d.W, PD_GROUPING_MAX_K);
        const int32_t tiles_x = (d.W + kTileW - 1) / kTileW, tiles_y = (d.H + kWaves - 1) / kWaves;
        e = LabelsEntry{d.scores, d.mask, d.labels, d.counts, d.K, d.h, d.w, d.Hi, d.Wi, d.H, d.W, tiles_x,
                        (float)d.h / (float)d.Hp, (float)d.w / (float)d.Wp, (float)d.Hi / (float)d.H, (float)d.Wi / (float)d.W, wg_begin};
        return (int64_t)tiles_x * tiles_y;
      });
  if (wgs <= 0) return (int)wgs;
  hipLaunchKernelGGL(scores_argmax_resized, dim3((unsigned)wgs), dim3(kThreads), 0, st, (const LabelsEntry *)table_device, count);
  return pd_check_launch("pd_scores_argmax_resized_u8");
}

extern "C" int pd_masks_resize_u8(const PdMaskResize *list, int32_t count, void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<ResizeEntry>(
      "pd_masks_resize_u8", list, count, true, table_host_pinned, table_device, st,
      [](const PdMaskResize &d, int i, ResizeEntry &e, int64_t wg_begin) -> int64_t {
        if (d.n < 0 || !sizes_ok(d.Hp, d.Wp, d.Hi, d.Wi, d.H, d.W) || (d.n > 0 && (!d.src || !d.dst || !d.area)))
          return pd_set_error(PD_ERR_INVALID_ARG,
                              "pd_masks_resize_u8: image %d: n=%d Hp=%d Wp=%d Hi=%d Wi=%d H=%d W=%d (n >= 0, Hi <= Hp, Wi <= Wp, non-null "
                              "pointers required)",
                              i, d.n, d.Hp, d.Wp, d.Hi, d.Wi, d.H, d.W);
        const int32_t tiles_x = (d.W + kTileW - 1) / kTileW, tiles_y = (d.H + kWaves * kResizeRows - 1) / (kWaves * kResizeRows);
        e = ResizeEntry{d.src, d.dst, d.area, d.n, d.Hp, d.Wp, d.Hi, d.Wi, d.H, d.W, tiles_x, tiles_y, 0,
                        (float)d.Hi / (float)d.H, (float)d.Wi / (float)d.W, wg_begin};
        return (int64_t)tiles_x * tiles_y * d.n;
      });
  if (wgs <= 0) return (int)wgs;
  hipLaunchKernelGGL(masks_resize, dim3((unsigned)wgs), dim3(kThreads), 0, st, (const ResizeEntry *)table_device, count);
  return pd_check_launch("pd_masks_resize_u8");
}
