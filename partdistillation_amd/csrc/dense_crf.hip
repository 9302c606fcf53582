// Dense-CRF mean field with box-truncated Gaussians (C-ABI and the mathematics in include/pd_dcrf.h).
//
// The bilateral message is the hot path: (2 R2 + 1)^2 pixel pairs per pixel and step.  A workgroup of 4 wavefronts owns a tile of 64 columns
// x 8 rows; a lane owns kPy = 4 pixels of one column (4 consecutive rows), so one neighbour read from LDS feeds 4 pairs, and L accumulators per
// pixel live in registers.  Two wavefronts share each group of 4 output rows, one taking the even source rows and one the odd ones, and add
// their partial sums through LDS at the end: a 640 x 640 image then gives every SIMD about 3 wavefronts, and one wavefront alone issues a
// vector instruction only every 4 cycles where two or more reach one per 2.  The source rows [tile - R2, tile + R2] are streamed through LDS a few at a time: per row a strip of tile width +
// 2 R2 columns, each column holding its packed colour and the L pre-multiplied values n_2(j) Q[l, j] side by side.  The column stride is odd, so
// the 64 lanes of a wavefront (consecutive columns) read and write distinct banks.  Columns outside the image are staged as zeros and rows
// outside it are never visited: every LDS index is in range for every tile position, whatever the image size.
// Per pair: 3 subtractions and 3 multiply-adds for the colour distance and the exponent, one v_exp_f32, L multiply-adds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_dcrf.h"
#include "pd_msda.h"                         // PD_OK / PD_ERR_*

namespace {

constexpr int kThreads = 256;                // the per-pixel kernels
constexpr int kWaves = 4, kBilThreads = 64 * kWaves;
constexpr int kSplit = 2;                    // wavefronts that share the source rows of one group of output rows (even rows / odd rows)
constexpr int kGroups = kWaves / kSplit;     // groups of output rows per workgroup
static_assert(kWaves % kSplit == 0 && (kSplit & (kSplit - 1)) == 0, "kSplit: a power of two that divides kWaves");
constexpr int kPy = 4;                       // pixels (rows) per lane of the bilateral kernel
constexpr int kTileW = 64, kTileH = kGroups * kPy;
constexpr int kLdsBudget = 40 * 1024;        // bytes of staged rows per workgroup: 4 workgroups fit a CU's 160 KB
constexpr int kMaxRows = 8;                  // most source rows staged at a time
constexpr float kLog2e = 1.4426950408889634f;

__host__ __device__ constexpr int stride_of(int LC) { return (1 + LC) | 1; }    // dwords per staged column: colour + LC values, made odd

struct Bilateral {
  const uint32_t *rgb;
  const uint8_t *lab;
  const float *n2;
  const float *q;
  const float *msg;
  float *out;                                // q_next [L, H, W], or n2 [H, W] for the pass over the field of ones
  int H, W, L, R, rows;
  float cs, cc;                              // log2(e) / (2 sd2^2), log2(e) / (2 sc^2)
  float u_same, u_other, compat2;            // -U for the pixel's own label and for the others
};

template <int LC, bool NORM>
__global__ void __launch_bounds__(kBilThreads) dcrf_bilateral(const Bilateral a)
{
  extern __shared__ float lds[];             // [rows][SW][stride]
  constexpr int ST = stride_of(LC);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W, L = a.L, R = a.R, HW = H * W;
  const int SW = kTileW + 2 * R, row_dwords = SW * ST;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int part = wave % kSplit, x = tx0 + lane, yw = ty0 + (wave / kSplit) * kPy;

  float cr[kPy], cg[kPy], cb[kPy];
#pragma unroll
  for (int k = 0; k < kPy; ++k) {
    const uint32_t c = (x < W && yw + k < H) ? a.rgb[(yw + k) * W + x] : 0u;
    cr[k] = (float)(c & 0xff), cg[k] = (float)((c >> 8) & 0xff), cb[k] = (float)((c >> 16) & 0xff);
    // keeps the differences below in fp32: knowing both sides are bytes, the compiler would subtract them as integers and convert every
    // difference (12 conversions per neighbour instead of 3)
    asm volatile("" : "+v"(cr[k]), "+v"(cg[k]), "+v"(cb[k]));
  }
  float acc[kPy][LC];
#pragma unroll
  for (int k = 0; k < kPy; ++k)
#pragma unroll
    for (int l = 0; l < LC; ++l) acc[k][l] = 0.f;

  const int r_begin = ty0 - R > 0 ? ty0 - R : 0;
  const int r_last = ty0 + kTileH - 1 + R < H - 1 ? ty0 + kTileH - 1 + R : H - 1;
  for (int r0 = r_begin; r0 <= r_last; r0 += a.rows) {
    const int nr = r_last - r0 + 1 < a.rows ? r_last - r0 + 1 : a.rows;
    __syncthreads();                                                             // the previous rows have been consumed
    for (int idx = tid; idx < nr * SW; idx += kBilThreads) {
      const int rr = idx / SW, s = idx - rr * SW;
      const int c = tx0 - R + s;
      const bool in = c >= 0 && c < W;
      const int g = (r0 + rr) * W + c;
      float *col = lds + rr * row_dwords + s * ST;
      col[0] = __uint_as_float(in ? a.rgb[g] : 0u);
      if constexpr (NORM) {
        col[1] = in ? 1.f : 0.f;
      } else {
        const float nn = in ? a.n2[g] : 0.f;
#pragma unroll
        for (int l = 0; l < LC; ++l) col[1 + l] = (in && l < L) ? nn * a.q[l * HW + g] : 0.f;
      }
    }
    __syncthreads();
    for (int rr = 0; rr < nr; ++rr) {
      const int r = r0 + rr;
      if ((r & (kSplit - 1)) != part) continue;                                  // the other wavefront of the group takes this row
      float sy[kPy];                                                             // -dy^2 cs, or -inf (a weight of 0) outside the box
      bool any = false;
#pragma unroll
      for (int k = 0; k < kPy; ++k) {
        const int dy = r - (yw + k);
        const bool ok = dy >= -R && dy <= R;
        sy[k] = ok ? -(float)(dy * dy) * a.cs : -INFINITY;
        any |= ok;
      }
      if (!any) continue;                                                        // wave-uniform: yw is
      const float *p = lds + rr * row_dwords + lane * ST;
#pragma unroll 2
      for (int d = 0; d <= 2 * R; ++d, p += ST) {
        const int dx = d - R;
        const float sx = -(float)(dx * dx) * a.cs;
        const uint32_t c = __float_as_uint(p[0]);
        const float nr_ = (float)(c & 0xff), ng = (float)((c >> 8) & 0xff), nb = (float)((c >> 16) & 0xff);
        float v[LC];
#pragma unroll
        for (int l = 0; l < LC; ++l) v[l] = p[1 + l];
#pragma unroll
        for (int k = 0; k < kPy; ++k) {
          const float dr = cr[k] - nr_, dg = cg[k] - ng, db = cb[k] - nb;
          float cd = dr * dr;
          cd = fmaf(dg, dg, cd);
          cd = fmaf(db, db, cd);
          const float w = __builtin_amdgcn_exp2f(fmaf(cd, -a.cc, sy[k] + sx));
#pragma unroll
          for (int l = 0; l < LC; ++l) acc[k][l] = fmaf(w, v[l], acc[k][l]);
        }
      }
    }
  }

  // the partial sums of a group meet in LDS (lanes side by side: no bank conflicts) and are added in a fixed order
  __syncthreads();                                                               // the last rows have been consumed
  if (part != 0) {
    float *red = lds + (((wave / kSplit) * (kSplit - 1) + part - 1) * kPy * LC) * 64 + lane;
#pragma unroll
    for (int k = 0; k < kPy; ++k)
#pragma unroll
      for (int l = 0; l < LC; ++l) red[(k * LC + l) * 64] = acc[k][l];
  }
  __syncthreads();
  if (part != 0) return;
#pragma unroll
  for (int q = 0; q < kSplit - 1; ++q) {
    const float *red = lds + (((wave / kSplit) * (kSplit - 1) + q) * kPy * LC) * 64 + lane;
#pragma unroll
    for (int k = 0; k < kPy; ++k)
#pragma unroll
      for (int l = 0; l < LC; ++l) acc[k][l] += red[(k * LC + l) * 64];
  }
#pragma unroll
  for (int k = 0; k < kPy; ++k) {
    const int y = yw + k;
    if (x >= W || y >= H) continue;
    const int g = y * W + x;
    if constexpr (NORM) {
      a.out[g] = 1.f / sqrtf(acc[k][0] + 1e-20f);
    } else {
      const float nn = a.compat2 * a.n2[g];
      const int lb = a.lab[g];
      float s[LC], m = -INFINITY;
#pragma unroll
      for (int l = 0; l < LC; ++l) {
        s[l] = -INFINITY;
        if (l < L) s[l] = (l == lb ? a.u_same : a.u_other) + a.msg[l * HW + g] + nn * acc[k][l];
        m = fmaxf(m, s[l]);
      }
      float sum = 0.f;
#pragma unroll
      for (int l = 0; l < LC; ++l) {
        s[l] = l < L ? expf(s[l] - m) : 0.f;
        sum += s[l];
      }
      const float inv = 1.f / sum;
#pragma unroll
      for (int l = 0; l < LC; ++l)
        if (l < L) a.out[l * HW + g] = s[l] * inv;
    }
  }
}

// exp(-d^2 / (2 sd^2)) for d = 0 .. R into LDS (R <= PD_DCRF_MAX_RADIUS)
__device__ __forceinline__ void fill_table(float *e, int R, float inv2s2)
{
  for (int d = threadIdx.x; d <= R; d += blockDim.x) e[d] = expf(-(float)(d * d) * inv2s2);
  __syncthreads();
}

// one thread per pixel: the packed colour, n_1 (the box sum of k1 factors into a row sum and a column sum) and Q_0
__global__ void __launch_bounds__(kThreads) dcrf_prepare(const uint8_t *image, const uint8_t *lab, int H, int W, int L, int R1, float inv2s2,
                                                         float q_same, float q_other, uint32_t *rgb, float *n1, float *q0)
{
  __shared__ float e[PD_DCRF_MAX_RADIUS + 1];
  fill_table(e, R1, inv2s2);
  const int g = blockIdx.x * kThreads + threadIdx.x, HW = H * W;
  if (g >= HW) return;
  const int y = g / W, x = g - y * W;
  const uint8_t *px = image + (size_t)3 * g;
  rgb[g] = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
  float sx = 0.f, sy = 0.f;
  for (int d = -R1; d <= R1; ++d) {
    const float w = e[d < 0 ? -d : d];
    sx += (x + d >= 0 && x + d < W) ? w : 0.f;
    sy += (y + d >= 0 && y + d < H) ? w : 0.f;
  }
  n1[g] = 1.f / sqrtf(sx * sy + 1e-20f);
  const int lb = lab[g];
  for (int l = 0; l < L; ++l) q0[l * HW + g] = l == lb ? q_same : q_other;
}

// rows: tmp[l, y, x] = sum_dx e[|dx|] n1[y, x + dx] q[l, y, x + dx]
__global__ void __launch_bounds__(kThreads) dcrf_spatial_rows(const float *q, const float *n1, int H, int W, int L, int R1, float inv2s2,
                                                              float *tmp)
{
  __shared__ float e[PD_DCRF_MAX_RADIUS + 1];
  fill_table(e, R1, inv2s2);
  const int i = blockIdx.x * kThreads + threadIdx.x, HW = H * W;
  if (i >= L * HW) return;
  const int l = i / HW, g = i - l * HW, x = g % W;
  const int lo = x - R1 > 0 ? -R1 : -x, hi = x + R1 < W ? R1 : W - 1 - x;
  float s = 0.f;
  for (int d = lo; d <= hi; ++d) s = fmaf(e[d < 0 ? -d : d], n1[g + d] * q[i + d], s);
  tmp[i] = s;
}

// columns: msg[l, y, x] = compat1 n1[y, x] sum_dy e[|dy|] tmp[l, y + dy, x]
__global__ void __launch_bounds__(kThreads) dcrf_spatial_cols(const float *tmp, const float *n1, int H, int W, int L, int R1, float inv2s2,
                                                              float compat1, float *msg)
{
  __shared__ float e[PD_DCRF_MAX_RADIUS + 1];
  fill_table(e, R1, inv2s2);
  const int i = blockIdx.x * kThreads + threadIdx.x, HW = H * W;
  if (i >= L * HW) return;
  const int l = i / HW, g = i - l * HW, y = g / W;
  const int lo = y - R1 > 0 ? -R1 : -y, hi = y + R1 < H ? R1 : H - 1 - y;
  float s = 0.f;
  for (int d = lo; d <= hi; ++d) s = fmaf(e[d < 0 ? -d : d], tmp[i + d * W], s);
  msg[i] = compat1 * n1[g] * s;
}

__global__ void __launch_bounds__(kThreads) dcrf_argmax(const float *q, int HW, int L, uint8_t *out)
{
  const int g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= HW) return;
  float best = q[g];
  int bi = 0;
  for (int l = 1; l < L; ++l) {
    const float v = q[l * HW + g];
    if (v > best) best = v, bi = l;
  }
  out[g] = (uint8_t)bi;
}

int radius_of(double sd) { return (int)ceil(3.0 * sd); }

// the checks every entry point shares
int check_shape(const char *what, int H, int W, int L, double sd)
{
  if (L < 2 || L > PD_DCRF_MAX_LABELS || H <= 0 || W <= 0 || (int64_t)L * H * W >= INT32_MAX)
    return pd_set_error(PD_ERR_INVALID_ARG, "%s: H=%d W=%d L=%d (H, W > 0, 2 <= L <= %d, L * H * W < 2^31 required)", what, H, W, L,
                        PD_DCRF_MAX_LABELS);
  if (!(sd > 0.0) || !(3.0 * sd <= (double)PD_DCRF_MAX_RADIUS))
    return pd_set_error(PD_ERR_INVALID_ARG, "%s: sigma %g (0 < sigma, ceil(3 sigma) <= %d required)", what, sd, PD_DCRF_MAX_RADIUS);
  return PD_OK;
}

int check_p(const char *what, double p)
{
  if (!(p > 0.0 && p < 1.0)) return pd_set_error(PD_ERR_INVALID_ARG, "%s: p=%g (0 < p < 1 required)", what, p);
  return PD_OK;
}

template <int LC, bool NORM>
void launch_bilateral(Bilateral a, hipStream_t st)
{
  const int row_bytes = (kTileW + 2 * a.R) * stride_of(LC) * (int)sizeof(float);
  int rows = kLdsBudget / row_bytes;
  a.rows = rows < 1 ? 1 : (rows > kMaxRows ? kMaxRows : rows);
  const size_t reduce_bytes = (size_t)kGroups * (kSplit - 1) * kPy * LC * 64 * sizeof(float);
  const size_t lds_bytes = (size_t)a.rows * row_bytes > reduce_bytes ? (size_t)a.rows * row_bytes : reduce_bytes;
  const dim3 grid((unsigned)((a.W + kTileW - 1) / kTileW), (unsigned)((a.H + kTileH - 1) / kTileH));
  hipLaunchKernelGGL((dcrf_bilateral<LC, NORM>), grid, dim3(kBilThreads), lds_bytes, st, a);
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" int pd_dcrf_prepare(const uint8_t *image, const uint8_t *lab, int32_t H, int32_t W, int32_t L, double p, double sd1, double sd2,
                               double sc, uint32_t *rgb, float *n1, float *n2, float *q0, void *stream)
{
  if (!image || !lab || !rgb || !n1 || !n2 || !q0) return pd_set_error(PD_ERR_INVALID_ARG, "pd_dcrf_prepare: null pointer");
  if (int rc = check_shape("pd_dcrf_prepare", H, W, L, sd1)) return rc;
  if (int rc = check_shape("pd_dcrf_prepare", H, W, L, sd2)) return rc;
  if (int rc = check_p("pd_dcrf_prepare", p)) return rc;
  if (!(sc > 0.0)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_dcrf_prepare: sc=%g (sc > 0 required)", sc);
  hipStream_t st = (hipStream_t)stream;
  // Q_0 = softmax(-U): exp(-U) is p for the pixel's label and (1 - p) / (L - 1) for each of the others
  const double other = (1.0 - p) / (L - 1), z = p + (L - 1) * other;
  hipLaunchKernelGGL(dcrf_prepare, dim3(blocks_for((int64_t)H * W)), dim3(kThreads), 0, st, image, lab, H, W, L, radius_of(sd1),
                     (float)(1.0 / (2.0 * sd1 * sd1)), (float)(p / z), (float)(other / z), rgb, n1, q0);
  if (int rc = pd_check_launch("pd_dcrf_prepare")) return rc;
  Bilateral a{rgb, lab, nullptr, nullptr, nullptr, n2, H, W, 1, radius_of(sd2), 0, (float)(kLog2e / (2.0 * sd2 * sd2)),
              (float)(kLog2e / (2.0 * sc * sc)), 0.f, 0.f, 0.f};
  launch_bilateral<1, true>(a, st);
  return pd_check_launch("pd_dcrf_prepare");
}

extern "C" int pd_dcrf_spatial_message(const float *q, const float *n1, int32_t H, int32_t W, int32_t L, double sd1, double compat1, float *tmp,
                                       float *msg, void *stream)
{
  if (!q || !n1 || !tmp || !msg) return pd_set_error(PD_ERR_INVALID_ARG, "pd_dcrf_spatial_message: null pointer");
  if (int rc = check_shape("pd_dcrf_spatial_message", H, W, L, sd1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int R1 = radius_of(sd1);
  const float inv2s2 = (float)(1.0 / (2.0 * sd1 * sd1));
  const unsigned blocks = blocks_for((int64_t)L * H * W);
  hipLaunchKernelGGL(dcrf_spatial_rows, dim3(blocks), dim3(kThreads), 0, st, q, n1, H, W, L, R1, inv2s2, tmp);
  if (int rc = pd_check_launch("pd_dcrf_spatial_message")) return rc;
  hipLaunchKernelGGL(dcrf_spatial_cols, dim3(blocks), dim3(kThreads), 0, st, (const float *)tmp, n1, H, W, L, R1, inv2s2, (float)compat1, msg);
  return pd_check_launch("pd_dcrf_spatial_message");
}

extern "C" int pd_dcrf_bilateral_update(const uint32_t *rgb, const uint8_t *lab, const float *n2, const float *q, const float *msg, int32_t H,
                                        int32_t W, int32_t L, double p, double sd2, double sc, double compat2, float *q_next, void *stream)
{
  if (!rgb || !lab || !n2 || !q || !msg || !q_next) return pd_set_error(PD_ERR_INVALID_ARG, "pd_dcrf_bilateral_update: null pointer");
  if (q == q_next) return pd_set_error(PD_ERR_INVALID_ARG, "pd_dcrf_bilateral_update: q_next aliases q");
  if (int rc = check_shape("pd_dcrf_bilateral_update", H, W, L, sd2)) return rc;
  if (int rc = check_p("pd_dcrf_bilateral_update", p)) return rc;
  if (!(sc > 0.0)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_dcrf_bilateral_update: sc=%g (sc > 0 required)", sc);
  Bilateral a{rgb, lab, n2, q, msg, q_next, H, W, L, radius_of(sd2), 0, (float)(kLog2e / (2.0 * sd2 * sd2)), (float)(kLog2e / (2.0 * sc * sc)),
              (float)log(p), (float)log((1.0 - p) / (L - 1)), (float)compat2};
  hipStream_t st = (hipStream_t)stream;
  if (L <= 4) launch_bilateral<4, false>(a, st);
  else if (L <= 8) launch_bilateral<8, false>(a, st);
  else launch_bilateral<16, false>(a, st);
  return pd_check_launch("pd_dcrf_bilateral_update");
}

extern "C" int pd_dcrf_argmax(const float *q, int32_t H, int32_t W, int32_t L, uint8_t *out, void *stream)
{
  if (!q || !out) return pd_set_error(PD_ERR_INVALID_ARG, "pd_dcrf_argmax: null pointer");
  if (int rc = check_shape("pd_dcrf_argmax", H, W, L, 1.0)) return rc;
  hipLaunchKernelGGL(dcrf_argmax, dim3(blocks_for((int64_t)H * W)), dim3(kThreads), 0, (hipStream_t)stream, q, H * W, L, out);
  return pd_check_launch("pd_dcrf_argmax");
}
