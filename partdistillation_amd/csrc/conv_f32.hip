// fp32 NHWC convolutions of the ResNet backbone on the exact-f32 matrix instruction (include/pd_conv_f32.h): f32 operands, f32
// accumulation on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain), no fp16 / bf16 planes, no library call, no floating-point atomics.
//
//   conv_f32_igemm<BN, STEM>   implicit GEMM  rows x N x (taps * channels),  128 x BN x 32 tiles through LDS (pitch 36 floats), 4 waves.
//       One kernel, three uses.  Forward: rows = output pixels, N = co, the A row of a K-step is 32 channels of ONE tap's input pixel
//       (ci % 64 == 0, so a K-step never straddles two taps), loaded as zero when the tap lies outside the image.  Input gradient,
//       stride 1: rows = input pixels, N = ci, taps mirrored, the [ci][k][k][co] filter.  Input gradient, stride 2: one launch per
//       parity class (iy & 1, ix & 1) of the input pixel — a class sees a fixed subset of the taps (3 x 3: 1, 2, 2 or 4 of the nine;
//       1 x 1: one tap for the even-even class and none for the other three, which then write their addend or zero).  STEM: the 7 x 7 / 2,
//       K = 147 padded to 160, gathered per element (ci = 3).  The MFMA chain joins a second accumulator every 8 K-steps (two-level sum:
//       the error follows the chain's length, not K).  Epilogue: * scale + bias + residual / addend, ReLU.
//   conv_f32_wgrad<T, STEM>    filter gradient  co x (tap, ci) x pixels,  T x T output tiles (T = 128 when ci and co allow, else 64),
//       16 pixels per LDS stage; both operands are NHWC rows with the channel on the lanes, so nothing is transposed.  The pixels are cut
//       into S <= 64 equal parts (wgrad_plan: a function of the sizes only); part s writes its sums to workspace[s].
//   conv_f32_wgrad_reduce      dw = scale[co] * (workspace[0] + workspace[1] + ... in ascending order).
//
// Register files (-Rpass-analysis=kernel-resource-usage, gfx950; scratch = 0 bytes/lane in every kernel; the occupancy column is the
// register file's, waves/SIMD, before the dynamic LDS of the igemm kernels is counted — __launch_bounds__(256, 2) is what they run at):
//   conv_f32_igemm<128, false>   VGPRs 236  AGPRs 0  SGPRs 74  LDS 73728 (dynamic)  occupancy 2
//   conv_f32_igemm< 64, false>   VGPRs 138  AGPRs 0  SGPRs 70  LDS 55296 (dynamic)  occupancy 3
//   conv_f32_igemm<128, true>    VGPRs 241  AGPRs 0  SGPRs 64  LDS 73728 (dynamic)  occupancy 2
//   conv_f32_igemm< 64, true>    VGPRs 162  AGPRs 0  SGPRs 58  LDS 55296 (dynamic)  occupancy 3
//   conv_f32_wgrad<128, false>   VGPRs 101  AGPRs 0  SGPRs 46  LDS 40960            occupancy 4
//   conv_f32_wgrad< 64, false>   VGPRs  45  AGPRs 0  SGPRs 48  LDS 24576            occupancy 6
//   conv_f32_wgrad< 64, true>    VGPRs  57  AGPRs 0  SGPRs 50  LDS 24576            occupancy 6
//   conv_f32_wgrad_reduce        VGPRs  14  AGPRs 0  SGPRs 26  LDS 0                occupancy 8
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_conv_f32.h"
#include "pd_msda.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BK = 32, PITCH = BK + 4;
constexpr int STEM_K = 147, STEM_ROW = 21, STEM_KT = 5;       // 7 * 7 * 3; one filter row = 7 taps x 3 channels, contiguous in NHWC; ceil(147 / 32)
constexpr int OUTSIDE = -(1 << 28);                           // source coordinate of a row past M: every tap of it is outside the image

struct IgemmArgs {
  const float *src, *w, *scale, *bias, *add;   // add (residual / addend) may alias out: no __restrict__ on either
  float *out;
  int M, N, ntn;                 // rows = (b, ry, rx), ry < Hc, rx < Wc; N = output channels; N tiles
  int Hc, Wc;
  int hs, ws, cs, ms;            // source image and its channels; source pixel of tap t = (ry * ms + oy(t), rx * ms + ox(t))
  int Ho, Wo, os, py, px;        // output image; output pixel = (b, ry * os + py, rx * os + px)
  int k, nty, ntx, d0y, d0x, dstep, o0y, o0x, ostep;    // tap (ty, tx): filter tap (d0y + ty dstep, d0x + tx dstep), offset (o0y + ty ostep, ..)
  int relu;
};

template <int BN, bool STEM>
__global__ __launch_bounds__(256, 2) void conv_f32_igemm(const IgemmArgs a)
{
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float(*As)[BM][PITCH] = reinterpret_cast<float(*)[BM][PITCH]>(smem);
  float(*Bs)[BN][PITCH] = reinterpret_cast<float(*)[BN][PITCH]>(smem + 2 * BM * PITCH);
  constexpr int TI = BN == 128 ? 2 : 1, NB = BN / 32;        // 32-row MFMA tiles per wave; B rows per staging thread
  const int m0 = (int)(blockIdx.x / a.ntn) * BM, n0 = (int)(blockIdx.x % a.ntn) * BN;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = BN == 128 ? (wave >> 1) * 64 : wave * 32, wn = BN == 128 ? (wave & 1) * 64 : 0;
  // global -> register staging: the thread covers rows lr + 32 j, K columns lk .. lk + 3 of both tiles
  const int lr = t >> 3, lk = (t & 7) * 4;
  int sy0[4], sx0[4], sb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = m0 + lr + 32 * j;
    sy0[j] = sx0[j] = OUTSIDE, sb[j] = 0;
    if (row < a.M) {
      const int q = row / a.Wc;
      sx0[j] = (row - q * a.Wc) * a.ms, sy0[j] = (q % a.Hc) * a.ms, sb[j] = q / a.Hc;
    }
  }
  const int cpt = a.cs >> 5;                                   // K-steps per tap
  const int ldw = STEM ? STEM_K : a.k * a.k * a.cs;
  float4 ra[4], rb[NB];
  auto gload = [&](int kt) {
    if constexpr (STEM) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kk = kt * BK + lk + e, dy = kk / STEM_ROW, r = kk - dy * STEM_ROW;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int sy = sy0[j] + dy - 3, sxr = (sx0[j] - 3) * 3 + r;          // row sy, float sxr of that row's wi * 3
          const bool ok = kk < STEM_K && (unsigned)sy < (unsigned)a.hs && sx0[j] != OUTSIDE && (unsigned)sxr < (unsigned)(a.ws * 3);
          (&ra[j].x)[e] = ok ? a.src[((int64_t)sb[j] * a.hs + sy) * a.ws * 3 + sxr] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int n = n0 + lr + 32 * j;
          (&rb[j].x)[e] = (kk < STEM_K && n < a.N) ? a.w[(int64_t)n * STEM_K + kk] : 0.f;
        }
      }
    } else {
      const int tap = kt / cpt, c0 = (kt - tap * cpt) * BK + lk;
      const int ty = tap / a.ntx, tx = tap - ty * a.ntx;
      const int oy = a.o0y + ty * a.ostep, ox = a.o0x + tx * a.ostep;
      const int wk = ((a.d0y + ty * a.dstep) * a.k + a.d0x + tx * a.dstep) * a.cs + c0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sy = sy0[j] + oy, sx = sx0[j] + ox;
        const bool ok = (unsigned)sy < (unsigned)a.hs && (unsigned)sx < (unsigned)a.ws;
        ra[j] = ok ? *reinterpret_cast<const float4 *>(a.src + (((int64_t)sb[j] * a.hs + sy) * a.ws + sx) * a.cs + c0) : make_float4(0, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int n = n0 + lr + 32 * j;
        rb[j] = n < a.N ? *reinterpret_cast<const float4 *>(a.w + (int64_t)n * ldw + wk) : make_float4(0, 0, 0, 0);
      }
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4 *>(&As[buf][lr + 32 * j][lk]) = ra[j];
#pragma unroll
    for (int j = 0; j < NB; ++j) *reinterpret_cast<float4 *>(&Bs[buf][lr + 32 * j][lk]) = rb[j];
  };
  // two levels of sums: the MFMA chain runs over `flush` K-steps (>= 256 products), then joins `tot` and starts again from zero, so
  // the rounding error grows with the chain's length, not with K (4608 for res5's 3 x 3); at most 64 partial sums whatever K
  f32x16 acc[TI][2], tot[TI][2];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = tot[i][j][e] = 0.f;

  const int KT = STEM ? STEM_KT : a.nty * a.ntx * cpt;        // 0 for a parity class that no tap reaches
  const int flush = max(8, (KT + 63) / 64);
  int since = 0;
  if (KT > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  const int fr = lane & 31, fk = (lane >> 5) * 4;
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) gload(kt + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 8; ++ks) {
      float4 fa[TI], fb[2];
#pragma unroll
      for (int i = 0; i < TI; ++i) fa[i] = *reinterpret_cast<const float4 *>(&As[buf][wm + i * 32 + fr][ks * 8 + fk]);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const float4 *>(&Bs[buf][wn + j * 32 + fr][ks * 8 + fk]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32((&fa[i].x)[e], (&fb[j].x)[e], acc[i][j], 0, 0, 0);
    }
    if (++since == flush || kt + 1 == KT) {
      since = 0;
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          tot[i][j] += acc[i][j];
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        }
    }
    if (kt + 1 < KT) lstore(buf ^ 1);
    __syncthreads();
  }
  // epilogue: C/D layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn + j * 32 + (lane & 31);
    if (col >= a.N) continue;
    const float sv = a.scale ? a.scale[col] : 1.f, bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row >= a.M) continue;
        int64_t opix = row;
        if (a.os != 1) {
          const int q = row / a.Wc;
          opix = ((int64_t)(q / a.Hc) * a.Ho + (q % a.Hc) * a.os + a.py) * a.Wo + (row - q * a.Wc) * a.os + a.px;
        }
        float v = tot[i][j][e] * sv + bv;
        if (a.add) v += a.add[opix * a.N + col];
        if (a.relu) v = fmaxf(v, 0.f);
        a.out[opix * a.N + col] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- filter gradient
constexpr int WS = 16;   // pixels per LDS stage

struct WgradArgs {
  const float *dz, *x;
  float *part;                   // workspace [split][co][K]
  int M, ho, wo, hi, wi, ci, co, k, stride, pad;
  int K, tiles_k, tiles, m_chunk;
};

template <int T, bool STEM>
__global__ __launch_bounds__(256, 2) void conv_f32_wgrad(const WgradArgs a)
{
  constexpr int P = T + 32;                                    // row pitch: lanes 32 .. 63 read the next pixel's row, 32 banks further on
  constexpr int TI = T / 64, TPR = T / 4, RPP = 256 / TPR, NP = WS / RPP;
  __shared__ __attribute__((aligned(16))) float Ys[2][WS][P];
  __shared__ __attribute__((aligned(16))) float Xs[2][WS][P];
  const int tile = (int)(blockIdx.x % a.tiles), split = (int)(blockIdx.x / a.tiles);
  const int n0 = (tile / a.tiles_k) * T, kt = tile % a.tiles_k;
  const int cpt = STEM ? 1 : a.ci / T, tap = kt / cpt, c0 = (kt - tap * cpt) * T;      // STEM: kt = a 64-wide slice of the 147 (dy, dx, c)
  const int dy = tap / a.k, dx = tap - dy * a.k;
  const int mb = split * a.m_chunk, me = min(a.M, mb + a.m_chunk);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wn = (wave >> 1) * (T / 2), wk = (wave & 1) * (T / 2);
  const int lr = t / TPR, lc = (t % TPR) * 4;
  float4 ry[NP], rx[NP];
  auto gload = [&](int m) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int p = m + lr + RPP * j;
      ry[j] = rx[j] = make_float4(0, 0, 0, 0);
      if (p >= me) continue;
      ry[j] = *reinterpret_cast<const float4 *>(a.dz + (int64_t)p * a.co + n0 + lc);
      const int q = p / a.wo, ox = p - q * a.wo, oy = q % a.ho, b = q / a.ho;
      if constexpr (STEM) {
        const int64_t base = (int64_t)b * a.hi * a.wi * 3;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kk = kt * T + lc + e, ky = kk / STEM_ROW, r = kk - ky * STEM_ROW;
          const int sy = oy * 2 + ky - 3, sxr = (ox * 2 - 3) * 3 + r;
          if (kk < STEM_K && (unsigned)sy < (unsigned)a.hi && (unsigned)sxr < (unsigned)(a.wi * 3))
            (&rx[j].x)[e] = a.x[base + (int64_t)sy * a.wi * 3 + sxr];
        }
      } else {
        const int sy = oy * a.stride + dy - a.pad, sx = ox * a.stride + dx - a.pad;
        if ((unsigned)sy < (unsigned)a.hi && (unsigned)sx < (unsigned)a.wi)
          rx[j] = *reinterpret_cast<const float4 *>(a.x + (((int64_t)b * a.hi + sy) * a.wi + sx) * a.ci + c0 + lc);
      }
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      *reinterpret_cast<float4 *>(&Ys[buf][lr + RPP * j][lc]) = ry[j];
      *reinterpret_cast<float4 *>(&Xs[buf][lr + RPP * j][lc]) = rx[j];
    }
  };
  f32x16 acc[TI][TI];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TI; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int steps = (me - mb + WS - 1) / WS;
  if (steps > 0) {
    gload(mb);
    lstore(0);
  }
  __syncthreads();
  const int fc = lane & 31, fm = lane >> 5;
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < steps) gload(mb + (s + 1) * WS);
#pragma unroll
    for (int kk = 0; kk < WS / 2; ++kk) {
      float fa[TI], fb[TI];
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        fa[i] = Ys[buf][2 * kk + fm][wn + i * 32 + fc];
        fb[i] = Xs[buf][2 * kk + fm][wk + i * 32 + fc];
      }
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (s + 1 < steps) lstore(buf ^ 1);
    __syncthreads();
  }
  float *part = a.part + (int64_t)split * a.co * a.K;
#pragma unroll
  for (int j = 0; j < TI; ++j) {
    const int col = (STEM ? kt * T : tap * a.ci + c0) + wk + j * 32 + (lane & 31);
    if (col >= a.K) continue;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = n0 + wn + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < a.co) part[(int64_t)row * a.K + col] = acc[i][j][e];
      }
  }
}

__global__ __launch_bounds__(256) void conv_f32_wgrad_reduce(const float *__restrict__ part, const float *__restrict__ scale,
                                                              float *__restrict__ dw, int64_t total, int K, int splits)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float s = part[i];
  for (int p = 1; p < splits; ++p) s += part[(int64_t)p * total + i];
  dw[i] = scale ? s * scale[i / K] : s;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

bool body_supported(int ci, int co, int k, int stride, int pad)
{
  return ci > 0 && co > 0 && ci % 64 == 0 && co % 64 == 0 && (k == 1 || k == 3) && (stride == 1 || stride == 2) && pad == k / 2;
}

// sizes every entry point checks: positive, the output size that belongs to the input size, a pixel count that fits an int
const char *bad_sizes(int batch, int hi, int wi, int ho, int wo, int k, int stride, int pad)
{
  if (batch < 0 || hi < 1 || wi < 1) return "batch >= 0, hi >= 1, wi >= 1 required";
  if (ho != (hi + 2 * pad - k) / stride + 1 || wo != (wi + 2 * pad - k) / stride + 1) return "ho, wo must be (size + 2 pad - k) / stride + 1";
  if ((int64_t)batch * hi * wi > 0x7fffffff / 4) return "more than 2^29 pixels";
  return nullptr;
}

template <bool STEM>
int igemm_launch(const IgemmArgs &a, hipStream_t s, const char *who)
{
  if (a.M == 0) return PD_OK;
  const bool wide = a.N % 128 == 0;
  const int bn = wide ? 128 : 64;
  IgemmArgs b = a;
  b.ntn = a.N / bn;
  const size_t lds = (size_t)2 * (BM + bn) * PITCH * sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void *)conv_f32_igemm<128, STEM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * (BM + 128) * PITCH * sizeof(float)));
    (void)hipFuncSetAttribute((const void *)conv_f32_igemm<64, STEM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * (BM + 64) * PITCH * sizeof(float)));
    attr = true;
  }
  const unsigned grid = (unsigned)(((int64_t)a.M + BM - 1) / BM * b.ntn);
  void (*kernel)(const IgemmArgs) = conv_f32_igemm<64, STEM>;
  if (wide) kernel = conv_f32_igemm<128, STEM>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, s, b);
  return pd_check_launch(who);
}

// the filter gradient's fixed partition: output tile edge, tiles, parts of the pixel sum and pixels per part — sizes only
struct WgradPlan {
  int T, tiles_k, tiles, splits, m_chunk;
};
WgradPlan wgrad_plan(int64_t M, int ci, int co, int k)
{
  WgradPlan p;
  const bool stem = ci == 3;
  p.T = !stem && ci % 128 == 0 && co % 128 == 0 ? 128 : 64;
  p.tiles_k = stem ? (STEM_K + 63) / 64 : k * k * (ci / p.T);
  p.tiles = (co / p.T) * p.tiles_k;
  int s = (1024 + p.tiles - 1) / p.tiles;       // ~4 workgroups per CU
  if (s > 64) s = 64;
  int64_t mc = ((M + s - 1) / s + WS - 1) / WS * WS;
  if (mc < 4 * WS) mc = 4 * WS;
  p.m_chunk = (int)mc;
  p.splits = (int)((M + mc - 1) / mc);
  return p;
}

int wgrad_launch(const float *dz, const float *x, const float *scale, float *dw, float *workspace, int64_t workspace_floats, int batch, int hi,
                 int wi, int ci, int ho, int wo, int co, int k, int stride, int pad, hipStream_t s, const char *who)
{
  const bool stem = ci == 3;
  const int K = k * k * ci;
  const int64_t M = (int64_t)batch * ho * wo, total = (int64_t)co * K;
  if (M == 0) {
    (void)hipMemsetAsync(dw, 0, (size_t)total * sizeof(float), s);
    return pd_check_launch(who);
  }
  const WgradPlan p = wgrad_plan(M, ci, co, k);
  if (!workspace || workspace_floats < p.splits * total) return pd_set_error(PD_ERR_INVALID_ARG, "%s: workspace of %lld floats needed", who, (long long)(p.splits * total));
  WgradArgs a = {dz, x, workspace, (int)M, ho, wo, hi, wi, ci, co, k, stride, pad, K, p.tiles_k, p.tiles, p.m_chunk};
  const dim3 grid((unsigned)(p.tiles * p.splits)), block(256);
  if (stem)
    hipLaunchKernelGGL((conv_f32_wgrad<64, true>), grid, block, 0, s, a);
  else if (p.T == 128)
    hipLaunchKernelGGL((conv_f32_wgrad<128, false>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((conv_f32_wgrad<64, false>), grid, block, 0, s, a);
  hipLaunchKernelGGL(conv_f32_wgrad_reduce, dim3((unsigned)((total + 255) / 256)), block, 0, s, workspace, scale, dw, total, K, p.splits);
  return pd_check_launch(who);
}

}  // namespace

extern "C" int pd_conv_f32_supported(int ci, int co, int k, int stride, int pad) { return body_supported(ci, co, k, stride, pad) ? 1 : 0; }

extern "C" int pd_conv_f32_fwd(const float *x, const float *w, const float *scale, const float *bias, const float *residual, float *y, int batch,
                               int hi, int wi, int ci, int ho, int wo, int co, int k, int stride, int pad, int relu, void *stream)
{
  if (!body_supported(ci, co, k, stride, pad))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_fwd: unsupported convolution ci %d co %d k %d stride %d pad %d", ci, co, k, stride, pad);
  if (const char *e = bad_sizes(batch, hi, wi, ho, wo, k, stride, pad)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_fwd: %s", e);
  if (!x || !w || !y || !aligned16(x) || !aligned16(w) || !aligned16(y) || !aligned16(residual))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_fwd: null or unaligned pointer");
  IgemmArgs a = {};
  a.src = x, a.w = w, a.scale = scale, a.bias = bias, a.add = residual, a.out = y;
  a.M = batch * ho * wo, a.N = co, a.Hc = ho, a.Wc = wo;
  a.hs = hi, a.ws = wi, a.cs = ci, a.ms = stride;
  a.Ho = ho, a.Wo = wo, a.os = 1;
  a.k = k, a.nty = a.ntx = k, a.dstep = 1, a.o0y = a.o0x = -pad, a.ostep = 1;
  a.relu = relu;
  return igemm_launch<false>(a, (hipStream_t)stream, "pd_conv_f32_fwd");
}

extern "C" int pd_conv_f32_dgrad(const float *dz, const float *wt, const float *addend, float *dx, int batch, int hi, int wi, int ci, int ho,
                                 int wo, int co, int k, int stride, int pad, void *stream)
{
  if (!body_supported(ci, co, k, stride, pad))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_dgrad: unsupported convolution ci %d co %d k %d stride %d pad %d", ci, co, k, stride, pad);
  if (const char *e = bad_sizes(batch, hi, wi, ho, wo, k, stride, pad)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_dgrad: %s", e);
  if (!dz || !wt || !dx || !aligned16(dz) || !aligned16(wt) || !aligned16(dx) || !aligned16(addend))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_dgrad: null or unaligned pointer");
  IgemmArgs a = {};
  a.src = dz, a.w = wt, a.add = addend, a.out = dx;
  a.N = ci, a.hs = ho, a.ws = wo, a.cs = co, a.ms = 1;
  a.Ho = hi, a.Wo = wi, a.k = k, a.ostep = -1;
  if (stride == 1) {
    a.M = batch * hi * wi, a.Hc = hi, a.Wc = wi, a.os = 1;
    a.nty = a.ntx = k, a.dstep = 1, a.o0y = a.o0x = pad;
    return igemm_launch<false>(a, (hipStream_t)stream, "pd_conv_f32_dgrad");
  }
  // stride 2: input pixel iy = 2 ry + py takes the filter taps dy with (py + pad - dy) even, from output row ry + (py + pad - dy) / 2
  a.os = 2, a.dstep = 2;
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px) {
      a.py = py, a.px = px;
      a.Hc = (hi - py + 1) / 2, a.Wc = (wi - px + 1) / 2;
      a.M = batch * a.Hc * a.Wc;
      a.d0y = (py + pad) & 1, a.d0x = (px + pad) & 1;
      a.nty = a.d0y < k ? (k - 1 - a.d0y) / 2 + 1 : 0, a.ntx = a.d0x < k ? (k - 1 - a.d0x) / 2 + 1 : 0;
      if (a.nty == 0 || a.ntx == 0) a.nty = a.ntx = 0;
      a.o0y = (py + pad - a.d0y) / 2, a.o0x = (px + pad - a.d0x) / 2;
      const int rc = igemm_launch<false>(a, (hipStream_t)stream, "pd_conv_f32_dgrad");
      if (rc != PD_OK) return rc;
    }
  return PD_OK;
}

extern "C" int64_t pd_conv_f32_wgrad_workspace_floats(int batch, int ho, int wo, int ci, int co, int k)
{
  if (batch < 1 || ho < 1 || wo < 1 || co < 64 || co % 64 || k < 1 || !((ci == 3 && k == 7) || (ci >= 64 && ci % 64 == 0))) return 0;
  return (int64_t)wgrad_plan((int64_t)batch * ho * wo, ci, co, k).splits * co * k * k * ci;
}

extern "C" int pd_conv_f32_wgrad(const float *dz, const float *x, const float *scale, float *dw, float *workspace, int64_t workspace_floats,
                                 int batch, int hi, int wi, int ci, int ho, int wo, int co, int k, int stride, int pad, void *stream)
{
  if (!body_supported(ci, co, k, stride, pad))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_wgrad: unsupported convolution ci %d co %d k %d stride %d pad %d", ci, co, k, stride, pad);
  if (const char *e = bad_sizes(batch, hi, wi, ho, wo, k, stride, pad)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_wgrad: %s", e);
  if (!dz || !x || !dw || !aligned16(dz) || !aligned16(x) || !aligned16(workspace))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv_f32_wgrad: null or unaligned pointer");
  return wgrad_launch(dz, x, scale, dw, workspace, workspace_floats, batch, hi, wi, ci, ho, wo, co, k, stride, pad, (hipStream_t)stream,
                      "pd_conv_f32_wgrad");
}

extern "C" int pd_stem7x7_f32_fwd(const float *x, const float *w, const float *scale, const float *bias, float *y, int batch, int hi, int wi,
                                  int ho, int wo, int co, int relu, void *stream)
{
  if (co < 64 || co % 64) return pd_set_error(PD_ERR_INVALID_ARG, "pd_stem7x7_f32_fwd: co %d is no multiple of 64", co);
  if (const char *e = bad_sizes(batch, hi, wi, ho, wo, 7, 2, 3)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_stem7x7_f32_fwd: %s", e);
  if (!x || !w || !y) return pd_set_error(PD_ERR_INVALID_ARG, "pd_stem7x7_f32_fwd: null pointer");
  IgemmArgs a = {};
  a.src = x, a.w = w, a.scale = scale, a.bias = bias, a.out = y;
  a.M = batch * ho * wo, a.N = co, a.Hc = ho, a.Wc = wo;
  a.hs = hi, a.ws = wi, a.cs = 3, a.ms = 2;
  a.Ho = ho, a.Wo = wo, a.os = 1, a.k = 7;
  a.relu = relu;
  return igemm_launch<true>(a, (hipStream_t)stream, "pd_stem7x7_f32_fwd");
}

extern "C" int pd_stem7x7_f32_wgrad(const float *dz, const float *x, const float *scale, float *dw, float *workspace, int64_t workspace_floats,
                                    int batch, int hi, int wi, int ho, int wo, int co, void *stream)
{
  if (co < 64 || co % 64) return pd_set_error(PD_ERR_INVALID_ARG, "pd_stem7x7_f32_wgrad: co %d is no multiple of 64", co);
  if (const char *e = bad_sizes(batch, hi, wi, ho, wo, 7, 2, 3)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_stem7x7_f32_wgrad: %s", e);
  if (!dz || !x || !dw || !aligned16(dz)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_stem7x7_f32_wgrad: null or unaligned pointer");
  return wgrad_launch(dz, x, scale, dw, workspace, workspace_floats, batch, hi, wi, 3, ho, wo, co, 7, 2, 3, (hipStream_t)stream,
                      "pd_stem7x7_f32_wgrad");
}
