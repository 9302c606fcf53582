// Device COCO run-length codec (include/pd_rle.h): uint8 planes -> run tables of their column-major flattenings, and run starts ->
// label map / masks.  Byte streams like the input pipeline's kernels; the point is that only run tables cross the bus.
//
// Planes -> runs, three launches, nothing waits and no atomic:
//   count   one wavefront per (plane, block of 64 columns, segment of SEG rows): lane = column, so every row read is one 64-byte segment; the
//           lane walks down its SEG rows and counts the pixels that differ from the pixel before them in COLUMN-major order (the pixel above;
//           for row 0 the bottom pixel of the column to the left; position 0 always starts a run).  Counts go to cnt[plane][xblock][seg][lane]
//           (lanes side by side: coalesced here, in the scan and in the write pass), the wavefront's sums of runs and of non-zero pixels to
//           wsum / wnz[plane][xblock][seg].
//   scan    one workgroup per (plane, xblock): its base = sum of wsum before it (64 x fewer entries than cnt, read redundantly instead of
//           handing a carry from workgroup to workgroup), then the exclusive scan of its [nseg][64] tile in key order (column, then segment):
//           column totals -> scan over the 64 lanes -> each thread walks its share of one column's segments.  In place.  The workgroups of
//           xblock 0 also write plane_offset and the plane's non-zero count (int64 sum of wnz).
//   write   the count pass again, storing (position, value) at the scanned offsets below `capacity`.
// pd_rle_masked_label_runs is the same three launches with another pixel fetch in the count / write pass: the plane's byte selects
// between a shared label map's byte and 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_msda.h"
#include "pd_rle.h"

namespace {
constexpr int SEG = PD_RLE_SEG_ROWS;
constexpr int PASS_WAVES = 4;                      // wavefronts (consecutive segments) per workgroup of the count / write pass
constexpr int SCAN_PARTS = 16;                     // wavefronts of a scan workgroup: each takes 1/16 of every column's segments
constexpr int MAX_GRID_Y = 65535;

__device__ __forceinline__ int wave_sum(int v)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the pixel fetch of the count / write pass: plane p's byte at row-major index i, or that of the virtual plane
// v[p][i] = planes[p][i] ? labels[i] : 0 (one label map under every plane; no such plane is ever written)
struct PlaneFetch {
  const uint8_t *__restrict__ planes;
  int64_t plane_stride;
  __device__ __forceinline__ int operator()(int p, int i) const { return planes[(int64_t)p * plane_stride + i]; }
};
struct MaskedLabelFetch {
  const uint8_t *__restrict__ planes;
  int64_t plane_stride;
  const uint8_t *__restrict__ labels;
  __device__ __forceinline__ int operator()(int p, int i) const { return planes[(int64_t)p * plane_stride + i] ? labels[i] : 0; }
};

template <bool WRITE, class Fetch>
__global__ __launch_bounds__(64 * PASS_WAVES) void plane_runs_pass(const Fetch px, int p0, int H, int W, int nseg, int XB, int SG, int binary,
                                                                   int32_t *__restrict__ cnt, int32_t *__restrict__ wsum,
                                                                   int32_t *__restrict__ wnz, int capacity, int32_t *__restrict__ run_start,
                                                                   uint8_t *__restrict__ run_value)
{
  const int lane = threadIdx.x & 63;
  const int xb = blockIdx.x / SG, s = (blockIdx.x % SG) * PASS_WAVES + (threadIdx.x >> 6);
  if (s >= nseg) return;                                                      // wave-uniform; the kernel has no barrier
  const int p = p0 + blockIdx.y, x = xb * 64 + lane, y0 = s * SEG;
  const int64_t key = ((int64_t)p * XB + xb) * nseg + s;
  int c = 0, nz = 0;
  if (x < W) {
    int b[SEG];
#pragma unroll
    for (int r = 0; r < SEG; ++r) b[r] = px(p, min(y0 + r, H - 1) * W + x);   // H * W <= 2^31 - 1: int indices
    int prev = -1;                                                            // position 0: no pixel before it, a run starts
    if (y0 > 0) prev = px(p, (y0 - 1) * W + x);
    else if (x > 0) prev = px(p, (H - 1) * W + x - 1);
    if (binary) prev = prev > 0 ? 1 : prev;
    int off = WRITE ? cnt[key * 64 + lane] : 0;
#pragma unroll
    for (int r = 0; r < SEG; ++r) {
      if (y0 + r < H) {
        const int v = binary ? (b[r] != 0) : b[r];
        if (v != prev) {
          if (WRITE) {
            if (off < capacity) { run_start[off] = x * H + y0 + r; run_value[off] = (uint8_t)v; }
            ++off;
          } else {
            ++c;
          }
        }
        nz += b[r] != 0;
        prev = v;
      }
    }
  }
  if (!WRITE) {
    cnt[key * 64 + lane] = c;                                                 // lanes past W too: the scan reads whole tiles
    c = wave_sum(c);
    nz = wave_sum(nz);
    if (lane == 0) { wsum[key] = c; wnz[key] = nz; }
  }
}

__global__ __launch_bounds__(64 * SCAN_PARTS) void plane_runs_scan(int32_t *__restrict__ cnt, const int32_t *__restrict__ wsum,
                                                                   const int32_t *__restrict__ wnz, int nseg, int XB, int n,
                                                                   int32_t *__restrict__ plane_offset, int64_t *__restrict__ plane_nonzero)
{
  __shared__ int part_sum[SCAN_PARTS][64];
  __shared__ int col_pre[64];
  __shared__ long long red[SCAN_PARTS];
  __shared__ int total;
  const int t = threadIdx.x, lane = t & 63, part = t >> 6;
  const int g = blockIdx.x, p = g / XB, xb = g % XB;
  // base: the runs of every (plane, xblock) before this one
  int acc = 0;
  for (int i = t; i < g * nseg; i += 64 * SCAN_PARTS) acc += wsum[i];
  acc = wave_sum(acc);
  if (lane == 0) red[part] = acc;
  __syncthreads();
  int base = 0;
  for (int q = 0; q < SCAN_PARTS; ++q) base += (int)red[q];
  __syncthreads();
  if (xb == 0) {                                                              // block-uniform
    long long z = 0;
    const int32_t *wz = wnz + (int64_t)p * XB * nseg;
    for (int i = t; i < XB * nseg; i += 64 * SCAN_PARTS) z += wz[i];
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
    if (lane == 0) red[part] = z;
    __syncthreads();
    if (t == 0) {
      z = 0;
      for (int q = 0; q < SCAN_PARTS; ++q) z += red[q];
      plane_nonzero[p] = z;
      plane_offset[p] = base;
    }
  }
  // exclusive scan of the [nseg][64] tile in key order: lane (column) major, segment minor
  const int per = (nseg + SCAN_PARTS - 1) / SCAN_PARTS, s0 = min(nseg, part * per), s1 = min(nseg, s0 + per);
  int32_t *c = cnt + (int64_t)g * nseg * 64 + lane;
  int sum = 0;
  for (int s = s0; s < s1; ++s) sum += c[(int64_t)s * 64];
  part_sum[part][lane] = sum;
  __syncthreads();
  if (part == 0) {
    int col = 0;
    for (int q = 0; q < SCAN_PARTS; ++q) col += part_sum[q][lane];
    int inc = col;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o);
      if (lane >= o) inc += v;
    }
    col_pre[lane] = inc - col;
    if (lane == 63) total = inc;
  }
  __syncthreads();
  int pre = base + col_pre[lane];
  for (int q = 0; q < part; ++q) pre += part_sum[q][lane];
  for (int s = s0; s < s1; ++s) {
    const int v = c[(int64_t)s * 64];
    c[(int64_t)s * 64] = pre;
    pre += v;
  }
  if (g == (int)gridDim.x - 1 && t == 0) plane_offset[n] = base + total;
}

// one thread per pixel, consecutive threads = consecutive x (coalesced stores); every mask's run starts are searched for the pixel's
// column-major position (neighbouring lanes search positions H apart)
__global__ __launch_bounds__(256) void rle_decode(const int32_t *__restrict__ starts, const int32_t *__restrict__ offsets, int n, int H, int W,
                                                  int32_t *__restrict__ labels, uint8_t *__restrict__ masks)
{
  const int64_t HW = (int64_t)H * W, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= HW) return;
  const int y = (int)(idx / W), x = (int)(idx % W), pos = x * H + y;
  int sum = 0;
  for (int i = 0; i < n; ++i) {
    const int o = offsets[i];
    const int v = pd_rle_find_run(starts + o, offsets[i + 1] - o, pos) & 1;
    sum += v * (i + 1);
    if (masks) masks[(int64_t)i * HW + idx] = (uint8_t)v;
  }
  if (labels) labels[idx] = sum;
}

// nseg, XB of a problem; false beyond the documented limits
bool runs_dims(int n, int H, int W, int *nseg, int *XB)
{
  if (n < 0 || H < 0 || W < 0 || (int64_t)H * W > 0x7fffffffLL || (int64_t)n * H * W > 0x7fffffffLL) return false;
  *nseg = (H + SEG - 1) / SEG;
  *XB = (W + 63) / 64;
  return (int64_t)n * *XB * *nseg * 64 <= 0x7fffffffLL;
}
// the three launches of pd_rle_plane_runs for either pixel fetch
template <class Fetch>
int plane_runs(const char *who, const Fetch &px, bool null_input, int n, int H, int W, int binary, int capacity, int32_t *run_start,
               uint8_t *run_value, int32_t *plane_offset, int64_t *plane_nonzero, void *workspace, void *stream_)
{
  int nseg, XB;
  if (capacity < 0 || px.plane_stride < 0 || !runs_dims(n, H, W, &nseg, &XB))
    return pd_set_error(PD_ERR_INVALID_ARG, "%s: bad sizes n=%d H=%d W=%d capacity=%d plane_stride=%lld", who, n, H, W, capacity,
                        (long long)px.plane_stride);
  if (!plane_offset || (n > 0 && !plane_nonzero)) return pd_set_error(PD_ERR_INVALID_ARG, "%s: null pointer", who);
  hipStream_t stream = (hipStream_t)stream_;
  if (n == 0 || H == 0 || W == 0) {                                            // no pixel, no run
    if (hipMemsetAsync(plane_offset, 0, sizeof(int32_t) * ((size_t)n + 1), stream) != hipSuccess ||
        (n > 0 && hipMemsetAsync(plane_nonzero, 0, sizeof(int64_t) * (size_t)n, stream) != hipSuccess))
      return pd_check_launch(who);
    return PD_OK;
  }
  if (null_input || !workspace || (capacity > 0 && (!run_start || !run_value))) return pd_set_error(PD_ERR_INVALID_ARG, "%s: null pointer", who);
  const int64_t keys = (int64_t)n * XB * nseg;
  int32_t *cnt = (int32_t *)workspace, *wsum = cnt + keys * 64, *wnz = wsum + keys;
  const int SG = (nseg + PASS_WAVES - 1) / PASS_WAVES;
  for (int p0 = 0; p0 < n; p0 += MAX_GRID_Y)
    hipLaunchKernelGGL((plane_runs_pass<false, Fetch>), dim3(XB * SG, n - p0 < MAX_GRID_Y ? n - p0 : MAX_GRID_Y), dim3(64 * PASS_WAVES), 0, stream,
                       px, p0, H, W, nseg, XB, SG, binary, cnt, wsum, wnz, 0, nullptr, nullptr);
  hipLaunchKernelGGL(plane_runs_scan, dim3(n * XB), dim3(64 * SCAN_PARTS), 0, stream, cnt, wsum, wnz, nseg, XB, n, plane_offset, plane_nonzero);
  if (capacity > 0)
    for (int p0 = 0; p0 < n; p0 += MAX_GRID_Y)
      hipLaunchKernelGGL((plane_runs_pass<true, Fetch>), dim3(XB * SG, n - p0 < MAX_GRID_Y ? n - p0 : MAX_GRID_Y), dim3(64 * PASS_WAVES), 0, stream,
                         px, p0, H, W, nseg, XB, SG, binary, cnt, wsum, wnz, capacity, run_start, run_value);
  return pd_check_launch(who);
}
}  // namespace

extern "C" int pd_rle_seg_rows(void) { return SEG; }

extern "C" int64_t pd_rle_runs_workspace_bytes(int n, int H, int W)
{
  int nseg, XB;
  if (!runs_dims(n, H, W, &nseg, &XB)) return -1;
  return (int64_t)n * XB * nseg * (64 + 2) * (int64_t)sizeof(int32_t);
}

extern "C" int pd_rle_plane_runs(const uint8_t *planes, int64_t plane_stride, int n, int H, int W, int binary, int capacity, int32_t *run_start,
                                 uint8_t *run_value, int32_t *plane_offset, int64_t *plane_nonzero, void *workspace, void *stream)
{
  return plane_runs("pd_rle_plane_runs", PlaneFetch{planes, plane_stride}, !planes, n, H, W, binary, capacity, run_start, run_value, plane_offset,
                    plane_nonzero, workspace, stream);
}

extern "C" int pd_rle_masked_label_runs(const uint8_t *planes, int64_t plane_stride, int n, int H, int W, const uint8_t *labels, int capacity,
                                        int32_t *run_start, uint8_t *run_value, int32_t *plane_offset, int64_t *plane_nonzero, void *workspace,
                                        void *stream)
{
  return plane_runs("pd_rle_masked_label_runs", MaskedLabelFetch{planes, plane_stride, labels}, !planes || !labels, n, H, W, 0, capacity,
                    run_start, run_value, plane_offset, plane_nonzero, workspace, stream);
}

extern "C" int pd_rle_decode(const int32_t *starts, const int32_t *offsets, int n, int H, int W, int32_t *labels, uint8_t *masks, void *stream_)
{
  if (n < 0 || H < 0 || W < 0 || (int64_t)H * W > 0x7fffffffLL)
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_rle_decode: bad sizes n=%d H=%d W=%d", n, H, W);
  if ((!labels && !masks) || (n > 0 && (!starts || !offsets))) return pd_set_error(PD_ERR_INVALID_ARG, "pd_rle_decode: null pointer");
  if (H == 0 || W == 0 || (n == 0 && !labels)) return PD_OK;
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(rle_decode, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, starts, offsets, n, H, W, labels, masks);
  return pd_check_launch("pd_rle_decode");
}
