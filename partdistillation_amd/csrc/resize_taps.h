// Bilinear source indices, taps and the packed 4-pixel accesses shared by the label-map / assignment kernels (grouping.hip,
// pixel_grouping.hip, mask_assign_resized.hip).  Every expression here is part of the numerics: the parentheses and the contraction
// setting of each function decide bits that the tests compare exactly.
#ifndef PD_RESIZE_TAPS_H
#define PD_RESIZE_TAPS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// Two rules for the same source index (torch upsample_bilinear2d, align_corners = false) exist on purpose:
//  - src_index is the form the compiler contracts (scale * (dst + 0.5) - 0.5 becomes one fma).  The full-size kernels
//    pd_scores_argmax_u8 and pd_mask_assign (grouping.hip) use it, and the identity branch of mask_assign_resized must reproduce
//    their bits, so it uses this very function.
//  - tap_of (below) rounds every step on its own, as ATen does; the resized kernels follow it.
__device__ __forceinline__ void src_index(int dst, float scale, int in_size, int &i0, int &ip, float &l0, float &l1)
{
  float src = scale * (dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  ip = (i0 < in_size - 1) ? 1 : 0;
  l1 = src - i0;
  l0 = 1.f - l1;
}

// the 2 x 2 bilinear value of src_index's taps: s[a] s[b] on the upper row, s[c] s[d] on the lower
__device__ __forceinline__ float bilinear2x2(const float *s, int a, int b, int c, int d, float hy0, float hy1, float wx0, float wx1)
{
  return hy0 * (wx0 * s[a] + wx1 * s[b]) + hy1 * (wx0 * s[c] + wx1 * s[d]);
}

// ATen's area_pixel_compute_source_index (align_corners = false) and the two taps of upsample_bilinear2d, every operation rounded on its
// own: contraction is switched off inside tap_of (HIP's default would fuse scale * (dst + 0.5) - 0.5 into one fma, and whether l1 is
// exactly 0 decides a mask pixel).  Every step is monotone, so the taps are non-decreasing in the output index: the column span of a
// run of pixels is [first tap of the first pixel, last tap of the last].
struct Tap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Tap tap_of(int dst, float scale, int in_size)
{
#pragma clang fp contract(off)
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  Tap t;
  t.i0 = (int)src;
  t.i0 = t.i0 < in_size - 1 ? t.i0 : in_size - 1;
  t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// the two chained interpolations along one axis: output index -> 4 low-resolution indices (i[0] the smallest, i[3] the largest; the
// middle two in no fixed order) and their weights
struct Tap4 {
  int i[4];
  float w[4];
};

__device__ __forceinline__ Tap4 chain_of(int dst, float scale2, int crop, float scale1, int low)
{
  const Tap o = tap_of(dst, scale2, crop);
  const Tap a = tap_of(o.i0, scale1, low), b = tap_of(o.i1, scale1, low);
  Tap4 t;
  t.i[0] = a.i0, t.i[1] = a.i1, t.i[2] = b.i0, t.i[3] = b.i1;
  t.w[0] = o.l0 * a.l0, t.w[1] = o.l0 * a.l1, t.w[2] = o.l1 * b.l0, t.w[3] = o.l1 * b.l1;
  return t;
}

// the 4 values at(i) of a Tap4's indices under its weights (rows first, then columns, in the kernels).  How a call site's lambda captures
// (by reference, by value, by name) moves the compiler's schedule, not the result: each site keeps the form whose code is that of the
// expression written out.
template <typename F>
__device__ __forceinline__ float mix4(const Tap4 &t, F at)
{
  return (t.w[0] * at(t.i[0]) + t.w[1] * at(t.i[1])) + (t.w[2] * at(t.i[2]) + t.w[3] * at(t.i[3]));
}

// ---- the 4 consecutive pixels of a lane: one packed access when all 4 are inside and the address allows it, guarded scalar accesses
// otherwise.  ok[j] says pixel j is inside (the callers have checked ok[0]); packed is the caller's `ok[3] && aligned4(p)` (aligned8 for
// int16), evaluated there: inside these functions the same test compiles to other code than it does in the kernel.
__device__ __forceinline__ bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }
__device__ __forceinline__ bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }

__device__ __forceinline__ void load4_u8(const uint8_t *p, bool packed, const bool (&ok)[4], uint8_t (&v)[4])
{
  if (packed) {
    const uint32_t x = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (uint8_t)(x >> (8 * j));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok[j]) v[j] = p[j];
  }
}

// byte j of x is pixel j
__device__ __forceinline__ void store4_u8(uint8_t *p, bool packed, const bool (&ok)[4], uint32_t x)
{
  if (packed) {
    *reinterpret_cast<uint32_t *>(p) = x;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok[j]) p[j] = (uint8_t)(x >> (8 * j));
  }
}

__device__ __forceinline__ uint32_t pack4_u8(const uint8_t (&v)[4])
{
  return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}

template <typename T>
__device__ __forceinline__ void store4_i16(int16_t *p, bool packed, const bool (&ok)[4], const T (&v)[4])
{
  if (packed) {
    uint2 x;
    x.x = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
    x.y = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
    *reinterpret_cast<uint2 *>(p) = x;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ok[j]) p[j] = (int16_t)v[j];
  }
}

}  // namespace
#endif
