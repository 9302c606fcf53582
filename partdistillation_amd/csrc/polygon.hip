// Polygon rasteriser (include/pd_poly.h): pycocotools' rleFrPoly restated as "every boundary position on its own".  Along an edge the
// upsampled column moves monotonically and by at most one per step, so the steps that cross from column 5X + 2 to 5X + 3 are known from
// the integer end points alone: a lane takes one such crossing, evaluates the two points around it exactly as the serial walk does
// (shallow edge: O(1); steep edge: a bisection for the step where the column changes) and writes its position.  The positions of a
// polygon are then sorted by its workgroup.  The work is a few hundred positions per polygon; the point is that it runs behind the
// image resample on the stream, with no host rasterisation and no dense mask upload.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"                                                    // pd_set_error, pd_check_launch
#include "pd_input.h"                                                     // PD_CANVAS_MAX_SIDE
#include "pd_msda.h"                                                      // PD_OK, PD_ERR_*
#include "pd_poly.h"
#include "poly_walk.h"                                                    // turns fp contraction off for this file

namespace {
constexpr int POLY_THREADS = 256, POLY_MAX_BLOCKS = 4096;

// ascending sort of a[0 .. n) by the whole workgroup: the bitonic network whose merges compare in ONE direction (the first step of a merge
// mirrors the upper half), so positions >= n act as +infinity without being stored: a comparator that reaches past n never swaps.
// Called and left with every thread's writes to `a` ordered by a barrier.
template <class T>
__device__ __forceinline__ void poly_sort(T *a, uint32_t n, uint32_t tid)
{
  uint32_t np = 1;
  while (np < n) np <<= 1;
  for (uint32_t s = 1; s < np; s <<= 1) {
    for (uint32_t d = s; d >= 1; d >>= 1) {
      for (uint32_t p = tid; p < np / 2; p += POLY_THREADS) {
        const uint32_t lo = 2 * p - (p & (d - 1));
        const uint32_t hi = d == s ? (lo | (2 * s - 1)) - (lo & (s - 1)) : lo + d;     // first step: lo's mirror inside the 2s block
        if (hi < n) {
          const T x = a[lo], y = a[hi];
          if (y < x) { a[lo] = y; a[hi] = x; }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(POLY_THREADS) void poly_crossings(const double *__restrict__ xy, const int32_t *__restrict__ vert_offsets, int n,
                                                               int h, int w, const int32_t *__restrict__ table_offsets, int32_t *starts)
{
  __shared__ int32_t lds[PD_POLY_LDS_ENTRIES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int poly = blockIdx.x; poly < n; poly += gridDim.x) {
    const int v0 = vert_offsets[poly], k = vert_offsets[poly + 1] - v0;
    const int t0 = table_offsets[poly];
    const int64_t cap = (int64_t)table_offsets[poly + 1] - t0 - 1;       // boundary positions the slice has room for
    if (cap < 0) continue;                                                // block-uniform
    int32_t *table = starts + t0;
    const bool in_lds = cap <= PD_POLY_LDS_ENTRIES;
    int32_t *buf = in_lds ? lds : table + 1;
    int64_t base = 0;                                                     // positions of the edges before this one (block-uniform)
    if (k > 0) {
      const double *v = xy + 2 * (int64_t)v0;
      const int first_x = poly_upsample(v[0]), first_y = poly_upsample(v[1]);
      int x1 = first_x, y1 = first_y;
      for (int j = 0; j < k; ++j) {                                       // every thread walks the vertex list: the counts are the offsets
        const int x0 = x1, y0 = y1;
        if (j + 1 < k) { x1 = poly_upsample(v[2 * (j + 1)]); y1 = poly_upsample(v[2 * (j + 1) + 1]); }
        else           { x1 = first_x; y1 = first_y; }
        const PolyColumns c = poly_edge_columns(x0, x1, w);
        if (c.count == 0) continue;
        if ((j & 3) == wave) {                                            // one wave per edge (it alone pays for the slope), lanes over its crossings
          const PolyEdge e = poly_edge(x0, y0, x1, y1);
          for (int q = lane; q < c.count; q += 64)
            if (base + q < cap) buf[base + q] = poly_crossing(e, c.first + q, h);
        }
        base += c.count;
      }
    }
    for (int64_t i = base + tid; i < cap; i += POLY_THREADS) buf[i] = 0x7fffffff;     // a slice longer than the polygon needs
    __syncthreads();
    poly_sort(buf, (uint32_t)cap, (uint32_t)tid);
    if (tid == 0) table[0] = 0;
    if (in_lds) {
      for (int i = tid; i < (int)cap; i += POLY_THREADS) table[1 + i] = lds[i];
      __syncthreads();                                                    // the next polygon reuses the buffer
    }
  }
}
}  // namespace

extern "C" int pd_poly_crossings_i32(const double *xy, const int32_t *vert_offsets, int n, int h, int w, const int32_t *table_offsets,
                                     int32_t *starts, void *stream_)
{
  if (n < 0 || h <= 0 || w <= 0 || h > PD_CANVAS_MAX_SIDE || w > PD_CANVAS_MAX_SIDE || (int64_t)h * w > 0x7fffffffLL)
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_poly_crossings_i32: bad sizes n=%d h=%d w=%d (sides 1..%d, h * w <= 2^31 - 1)", n, h, w,
                        PD_CANVAS_MAX_SIDE);
  if (n == 0) return PD_OK;
  if (!xy || !vert_offsets || !table_offsets || !starts) return pd_set_error(PD_ERR_INVALID_ARG, "pd_poly_crossings_i32: null pointer");
  const unsigned grid = (unsigned)(n < POLY_MAX_BLOCKS ? n : POLY_MAX_BLOCKS);
  hipLaunchKernelGGL(poly_crossings, dim3(grid), dim3(POLY_THREADS), 0, (hipStream_t)stream_, xy, vert_offsets, n, h, w, table_offsets, starts);
  return pd_check_launch("pd_poly_crossings_i32");
}
