// fp32 weight gradients on the bf16 / fp16 matrix cores.  Three-plane form: every fp32 operand element is split EXACTLY into
// three bf16 values
//     x = hi + mid + lo,   hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)     (3 x 8 significand bits = fp32's 24)
// when a tile is staged in LDS, and a product a*b is accumulated in fp32 as six bf16 MFMA terms
//     lo_a hi_b + hi_a lo_b + mid_a mid_b + mid_a hi_b + hi_a mid_b + hi_a hi_b
// (each bf16 x bf16 product is exact in fp32; the three dropped terms mid*lo, lo*mid, lo*lo are <= 2^-23 |a b| together —
// the size of ONE fp32 rounding of the product).  v_mfma_f32_32x32x16_bf16 runs 16 x the rate of v_mfma_f32_32x32x2_f32,
// so six of them per step are 2.7x the exact-fp32 matrix rate (measured against fp64 in tests/test_gemm_gpu.py: error at the
// level of the library's fp32 GEMM).  Two-plane form (H2): the fp16 split of f16x2.h, three products per term.
// The forward / input-gradient products that once lived here in the three-plane form (128 x 128 and 256 x 256 tiles, ReLU-bit and
// pre-split epilogues) are retired: gemm_f16x2.hip carries every such product.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f16x2.h"
#include "mfma_bf16.h"
#include "pd_common.h"
#include "xcd.h"
#include "pd_gemm.h"
#include "pd_msda.h"

namespace {
using namespace pdmfma;

constexpr int BM = 128, BN = 128;                                // output tile of the 128 x 128 kernels

struct Split4 { uint2 hi, mid, lo; };                            // 4 consecutive k of one row, per plane

__device__ __forceinline__ void split2(float x0, float x1, unsigned &h, unsigned &m, unsigned &l)
{
  h = pk_bf16(x0, x1);
  const float r0 = x0 - bf_lo(h), r1 = x1 - bf_hi(h);           // exact (Sterbenz / leading bits cancel)
  m = pk_bf16(r0, r1);
  l = pk_bf16(r0 - bf_lo(m), r1 - bf_hi(m));                    // the remainder has <= 8 significant bits: exact
}
__device__ __forceinline__ Split4 split4(float4 v)
{
  Split4 s;
  split2(v.x, v.y, s.hi.x, s.mid.x, s.lo.x);
  split2(v.z, v.w, s.hi.y, s.mid.y, s.lo.y);
  return s;
}
typedef __bf16 hwbf16x8 __attribute__((ext_vector_type(8)));   // operand of v_mfma_f32_32x32x16_bf16: 8 consecutive contraction elements per lane
__device__ __forceinline__ void mma16k(f32x16 &c, hwbf16x8 x, hwbf16x8 y) { c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, c, 0, 0, 0); }

__device__ __forceinline__ int xcd_chunk(int bid, int nb) { return pd_xcd_chunk(bid, nb); }   // xcd.h: any workgroup count

__device__ int g_wgrad_xcd = 1;   // tools only (pd_debug_set "wgrad_xcd" 0: launch order = logical order)
__device__ int g_wgrad_fast = 1;  // tools only (pd_debug_set "wgrad_fast" 0: the guarded step everywhere)

// ---------------------------------------------------------------------------------------------- weight gradient
// dW[N,K] += dY[M,N]^T X[M,K] contracts over the ROWS, so an MFMA operand (8 consecutive contraction elements per lane) is
// 8 consecutive rows of one column: the tiles are staged TRANSPOSED, [column][row pair] with the two rows of a pair packed
// in one dword (they are the low / high bf16 of the pair's split).  A lane stages one column (scalar 4-byte loads, 256
// contiguous bytes per wave instruction) so the 32 lanes of a write hit 32 different banks (row pitch 9 dwords, odd).
constexpr int WS = 16, WPD = WS / 2 + 1;                         // rows per stage, dwords per LDS row

__global__ __launch_bounds__(256, 2) void gemm_wgrad_f32x3(const float *__restrict__ dY, const float *__restrict__ X,
                                                            float *__restrict__ dW, float *__restrict__ dB, int M, int N, int K,
                                                            int ldy, int ldx, int ldw, int tiles_k, int tiles, int m_chunk)
{
  __shared__ unsigned Yt[2][3][BN][WPD];
  __shared__ unsigned Xt[2][3][BM][WPD];
  const int tile = blockIdx.x % tiles, split = blockIdx.x / tiles;
  const int n0 = (tile / tiles_k) * BN, k0 = (tile % tiles_k) * BM;
  const int mb = split * m_chunk, me = min(M, mb + m_chunk);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;
  const int col = t & 127, pg = (t >> 7) * 4;                    // this thread: column `col`, row pairs pg .. pg+3 of the stage
  const bool ycol_ok = n0 + col < N, xcol_ok = k0 + col < K;
  float ry[2][8], rx[2][8];                                      // two register stages
  auto gload = [&](int s, int m) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = m + 2 * pg + q;
      ry[s][q] = (r < me && ycol_ok) ? dY[(int64_t)r * ldy + n0 + col] : 0.f;
      rx[s][q] = (r < me && xcol_ok) ? X[(int64_t)r * ldx + k0 + col] : 0.f;
    }
  };
  const bool do_bias = dB != nullptr && k0 == 0;
  float bsum = 0.f;
  auto lstore = [&](int s, int buf) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned h, m_, l;
      split2(ry[s][2 * q], ry[s][2 * q + 1], h, m_, l);
      Yt[buf][0][col][pg + q] = h; Yt[buf][1][col][pg + q] = m_; Yt[buf][2][col][pg + q] = l;
      split2(rx[s][2 * q], rx[s][2 * q + 1], h, m_, l);
      Xt[buf][0][col][pg + q] = h; Xt[buf][1][col][pg + q] = m_; Xt[buf][2][col][pg + q] = l;
      if (do_bias) bsum += ry[s][2 * q] + ry[s][2 * q + 1];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int steps = (me - mb + WS - 1) / WS;
  if (steps > 0) {
    gload(0, mb);
    if (steps > 1) gload(1, mb + WS);
    lstore(0, 0);
  }
  __syncthreads();
  const int fr = lane & 31, fd = (lane >> 5) * 4;                // operand: column fr of a 32-block, row pairs fd .. fd+3 (8 rows)
  auto frag4 = [&](const unsigned *p) {
    union { unsigned d[4]; hwbf16x8 v; } u;
    u.d[0] = p[0]; u.d[1] = p[1]; u.d[2] = p[2]; u.d[3] = p[3];
    return u.v;
  };
  auto step = [&](int st, int par) {
    hwbf16x8 a[3][2], b[3][2];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[p][i] = frag4(&Yt[par][p][wn + i * 32 + fr][fd]);
        b[p][i] = frag4(&Xt[par][p][wk + i * 32 + fr][fd]);
      }
#define TERM(PA, PB)                                                         \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                              \
      _Pragma("unroll") for (int j = 0; j < 2; ++j) mma16k(acc[i][j], a[PA][i], b[PB][j]);
    TERM(2, 0) TERM(0, 2) TERM(1, 1) TERM(1, 0) TERM(0, 1) TERM(0, 0)
#undef TERM
    if (st + 1 < steps) lstore(par ^ 1, par ^ 1);
    if (st + 2 < steps) gload(par, mb + (st + 2) * WS);
    __syncthreads();
  };
  for (int st = 0; st < steps; st += 2) {
    step(st, 0);
    if (st + 1 < steps) step(st + 1, 1);
  }
  if (do_bias && ycol_ok) unsafeAtomicAdd(dB + n0 + col, bsum);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = k0 + wk + j * 32 + (lane & 31);
    if (c >= K) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = n0 + wn + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < N) unsafeAtomicAdd(dW + (int64_t)row * ldw + c, acc[i][j][e]);
      }
  }
}

// ---------------------------------------------------------------------------------------------- weight gradient, transpose-read form
// The same product with the tiles staged the way they lie in memory — [contraction row][column], 16-byte global loads, one
// 8-byte LDS write per plane — and TRANSPOSED ON THE WAY OUT of LDS by ds_read_b64_tr_b16 (gfx950): within a group of 16
// lanes, lane i receives element i % 4 of the 8-byte segments addressed by lanes i / 4 + 4 e (e = 0..3 -> the 4 result
// elements; mapping read off the hardware with tools/probes/tr_read_probe.hip).  Lane s of a group therefore points at
// row s / 4, columns 4 (s % 4) .. +3 of a [4 rows][16 columns] block and lane i gets column i of the 4 rows: two such reads are the
// 8 consecutive contraction elements of one column that v_mfma_f32_32x32x16_bf16 wants from lane (column, k half).
// Row pitch 160 bf16 = 320 bytes: the 4 rows of a read start 16 banks apart, its 32 lanes cover 64 distinct banks.
constexpr int TWS = 16, TP = 160;
typedef short v4s16 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ hwbf16x8 frag_tr(const bf16_t *p)      // p: this lane's segment of rows 0..3; rows 4..7 are 4 * TP further
{
  typedef __attribute__((address_space(3))) v4s16 *lp;
  union { v4s16 h[2]; hwbf16x8 v; } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(p));
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(p + 4 * TP));
  return u.v;
}

// CONV: X is an NHWC image [*, H, W, Ci] (ldx = Ci), K = 9 Ci ordered (tap, channel) like the channels-last filter gradient
// [Co][3][3][Ci]; Ci % 128 == 0, so a tile's 128 columns lie inside one tap and its X rows are the pixels m + dy W + dx (zeros
// outside the image): the weight gradient of a 3 x 3, stride 1, pad 1 convolution, nothing unfolded.
// H2: the fp16 two-plane form (f16x2.h; three products per term instead of six).  The contraction runs over the rows, so the two
// operands are scaled per WORKGROUP: by powers of two from the largest row maximum (y_amax / x_amax, the absolute row maxima of dY
// / X as their producers emit them; NULL = O(1) operand) among the rows [mb, me) this workgroup walks, undone on its partial tile.
// Rows far below their slab's maximum lose relative, not absolute, accuracy — the sum is dominated by the large rows.
template <int ABL, bool CONV, bool H2 = false>
__device__ __forceinline__ void wgrad_tr_body(const float *__restrict__ dY, const float *__restrict__ X, float *__restrict__ dW,
                                              float *__restrict__ dB, float *__restrict__ ws, int M, int N, int K, int ldy, int ldx,
                                              int ldw, int tiles_k, int tiles, int m_chunk, int H, int W, int bid, int64_t ws_tile0,
                                              const float *__restrict__ y_amax = nullptr, const float *__restrict__ x_amax = nullptr)
{
  constexpr int NP = H2 ? 2 : 3;
  __shared__ __attribute__((aligned(16))) bf16_t S[2][2][NP][TWS][TP];     // stage, operand (dY, X), plane, row, column
  const int tile = bid % tiles, split = bid / tiles;
  const int n0 = (tile / tiles_k) * BN, k0 = (tile % tiles_k) * BM;
  const int mb = split * m_chunk, me = min(M, mb + m_chunk);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;
  const int sr = t >> 5, sc = (t & 31) * 4;                      // staging: rows sr, sr + 8; columns sc .. sc+3
  const bool ycol_ok = n0 + sc < N, xcol_ok = k0 + sc < K;
  float sy = 1.f, sx = 1.f, inv_yx = 1.f;
  if (H2 && (y_amax || x_amax)) {
    float my = 0.f, mx = 0.f;
    if (y_amax) for (int r = mb + t; r < me; r += 256) my = fmaxf(my, y_amax[r]);
    // CONV: the X rows of this slab are the pixels r + dy W + dx — the range widened by one image row + 1 bounds them
    const int xlo = CONV ? max(0, mb - W - 1) : mb, xhi = CONV ? min(M, me + W + 1) : me;
    if (x_amax) for (int r = xlo + t; r < xhi; r += 256) mx = fmaxf(mx, x_amax[r]);
#pragma unroll
    for (int o = 32; o; o >>= 1) { my = fmaxf(my, __shfl_xor(my, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
    float *red = reinterpret_cast<float *>(&S[0][0][0][0][0]);
    if (lane == 0) { red[wave] = my; red[4 + wave] = mx; }
    __syncthreads();
    my = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    __syncthreads();
    float iy = 1.f, ix = 1.f;
    if (y_amax) pdh2::row_scale(my, sy, iy);
    if (x_amax) pdh2::row_scale(mx, sx, ix);
    inv_yx = iy * ix;
  }
  float4 ry[2][2], rx[2][2];                                     // two register stages
  int cpy[2] = {0, 0}, cpx[2] = {0, 0}, tdy = 0, tdx = 0, xoff = k0 + sc;   // CONV: image coordinates of the rows the NEXT gload stages
  if (CONV) {
    const int tap = k0 / ldx;
    tdy = tap / 3 - 1; tdx = tap - (tap / 3) * 3 - 1;
    xoff = k0 - tap * ldx + sc;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int pix = (mb + sr + 8 * j) % (H * W);
      cpy[j] = pix / W; cpx[j] = pix - cpy[j] * W;
    }
  }
  auto gload = [&](int s, int m) {                               // called with m = mb, mb + 16, mb + 32, ... in this order
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = m + sr + 8 * j;
      ry[s][j] = (r < me && ycol_ok) ? *reinterpret_cast<const float4 *>(dY + (int64_t)r * ldy + n0 + sc) : make_float4(0, 0, 0, 0);
      if (CONV) {
        const int yy = cpy[j] + tdy, xx = cpx[j] + tdx;
        const bool ok = r < me && xcol_ok && yy >= 0 && yy < H && xx >= 0 && xx < W;
        rx[s][j] = ok ? *reinterpret_cast<const float4 *>(X + ((int64_t)r + tdy * W + tdx) * ldx + xoff) : make_float4(0, 0, 0, 0);
        cpx[j] += TWS;
        while (cpx[j] >= W) { cpx[j] -= W; if (++cpy[j] == H) cpy[j] = 0; }
      } else {
        rx[s][j] = (r < me && xcol_ok) ? *reinterpret_cast<const float4 *>(X + (int64_t)r * ldx + k0 + sc) : make_float4(0, 0, 0, 0);
      }
    }
  };
  const bool do_bias = dB != nullptr && k0 == 0;
  float4 bsum = make_float4(0, 0, 0, 0);
  auto lstore = [&](int s, int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = sr + 8 * j;
      if constexpr (H2) {
        const pdh2::SplitH y = pdh2::split4h(ry[s][j], sy), x = pdh2::split4h(rx[s][j], sx);
        *reinterpret_cast<uint2 *>(&S[buf][0][0][r][sc]) = y.hi; *reinterpret_cast<uint2 *>(&S[buf][0][1][r][sc]) = y.lo;
        *reinterpret_cast<uint2 *>(&S[buf][1][0][r][sc]) = x.hi; *reinterpret_cast<uint2 *>(&S[buf][1][1][r][sc]) = x.lo;
      } else {
        const Split4 y = split4(ry[s][j]), x = split4(rx[s][j]);
        *reinterpret_cast<uint2 *>(&S[buf][0][0][r][sc]) = y.hi; *reinterpret_cast<uint2 *>(&S[buf][0][1][r][sc]) = y.mid;
        *reinterpret_cast<uint2 *>(&S[buf][0][NP - 1][r][sc]) = y.lo;
        *reinterpret_cast<uint2 *>(&S[buf][1][0][r][sc]) = x.hi; *reinterpret_cast<uint2 *>(&S[buf][1][1][r][sc]) = x.mid;
        *reinterpret_cast<uint2 *>(&S[buf][1][NP - 1][r][sc]) = x.lo;
      }
      if (do_bias) { bsum.x += ry[s][j].x; bsum.y += ry[s][j].y; bsum.z += ry[s][j].z; bsum.w += ry[s][j].w; }
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int steps = (me - mb + TWS - 1) / TWS;
  if (steps > 0) {
    gload(0, mb);
    if (steps > 1) gload(1, mb + TWS);
    lstore(0, 0);
  }
  __syncthreads();
  const int grp = lane >> 4, sl = lane & 15;
  const int frow = 8 * (grp >> 1) + (sl >> 2), fcol = 16 * (grp & 1) + 4 * (sl & 3);   // this lane's segment inside a 32-column block
  auto step = [&](int st, int par) {
    if (st + 2 < steps) gload(par, mb + (st + 2) * TWS);
    hwbf16x8 a[NP][2], b[NP][2];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[p][i] = frag_tr(&S[par][0][p][frow][wn + i * 32 + fcol]);
        b[p][i] = frag_tr(&S[par][1][p][frow][wk + i * 32 + fcol]);
      }
#define TERM(PA, PB)                                                         \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                              \
      _Pragma("unroll") for (int j = 0; j < 2; ++j) {                        \
        if constexpr (H2) pdh2::mmah(acc[i][j], __builtin_bit_cast(pdh2::h16x8, a[PA][i]), __builtin_bit_cast(pdh2::h16x8, b[PB][j])); \
        else mma16k(acc[i][j], a[PA][i], b[PB][j]);                          \
      }
    if constexpr (H2) { TERM(1, 0) TERM(0, 1) TERM(0, 0) }
    else if (ABL != 2) { TERM(NP - 1, 0) TERM(0, NP - 1) TERM(1, 1) TERM(1, 0) TERM(0, 1) TERM(0, 0) }
    else { _Pragma("unroll") for (int p = 0; p < NP; ++p) _Pragma("unroll") for (int i = 0; i < 2; ++i) { acc[i][0][p] += (float)a[p][i][0]; acc[i][1][p] += (float)b[p][i][0]; } }
#undef TERM
    if (st + 1 < steps) lstore(par ^ 1, par ^ 1);
    __syncthreads();
  };
  for (int st = 0; st < steps; st += 2) {
    step(st, 0);
    if (st + 1 < steps) step(st + 1, 1);
  }
  if (do_bias) {
    // column sums: the 8 staging rows of a column are summed through LDS first — ONE atomic per column and workgroup (8 x splits
    // same-address atomics per column serialise: 1 024 of them cost ~100 us at 256 x 256)
    float *red = reinterpret_cast<float *>(&S[0][0][0][0][0]);   // the last step ended with a barrier: the stages are free
    *reinterpret_cast<float4 *>(red + sr * BN + sc) = bsum;
    __syncthreads();
    if (t < BN && n0 + t < N) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) v += red[r * BN + t];
      unsafeAtomicAdd(dB + n0 + t, v);
    }
  }
  if (ws) {
    // partial tile in REGISTER order (element (ij, e) of thread t at ((ij * 16 + e) * 256 + t): 1 KB per store instruction);
    // wgrad_tr_reduce sums the splits and owns the read-modify-write of dW — 8.4 M fp32 atomics per launch cost 30-110 us
    float *w = ws + (ws_tile0 + (int64_t)split * tiles + tile) * (BN * BM) + t;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) w[((i * 2 + j) * 16 + e) * 256] = H2 ? acc[i][j][e] * inv_yx : acc[i][j][e];
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = k0 + wk + j * 32 + (lane & 31);
    if (c >= K) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = n0 + wn + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < N) unsafeAtomicAdd(dW + (int64_t)row * ldw + c, H2 ? acc[i][j][e] * inv_yx : acc[i][j][e]);
      }
  }
}

template <int ABL, bool CONV, bool H2 = false>
__global__ __launch_bounds__(256, 2) void gemm_wgrad_f32x3_tr(const float *__restrict__ dY, const float *__restrict__ X,
                                                               float *__restrict__ dW, float *__restrict__ dB, float *__restrict__ ws,
                                                               int M, int N, int K, int ldy, int ldx, int ldw, int tiles_k, int tiles,
                                                               int m_chunk, int H, int W, const float *__restrict__ y_amax,
                                                               const float *__restrict__ x_amax)
{
  // XCD-aware order (block i runs on XCD i % 8): the output tiles of one slab of rows are consecutive LOGICAL blocks, i.e. land on
  // the same XCD at about the same time and share the slab's dY / X columns in its L2 instead of fetching them into all eight
  const int lb = g_wgrad_xcd ? xcd_chunk((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  wgrad_tr_body<ABL, CONV, H2>(dY, X, dW, dB, ws, M, N, K, ldy, ldx, ldw, tiles_k, tiles, m_chunk, H, W, lb, 0, y_amax, x_amax);
}

// ---------------------------------------------------------------------------------------------- weight gradient, 256 x 256 tiles (f16x2)
// The 128 x 128 kernel above re-reads every slab of rows once per output tile that needs its columns: 2.8 x the algorithmic bytes
// at the encoder's five weight gradients (rocprofv3 FETCH_SIZE / WRITE_SIZE: 1.97 GB per layer against 0.71 GB, profiles/r03_gemm_pmc.json) —
// 11.8 GB per step in 1.6 ms, i.e. the kernel runs at the memory system's limit ON ITS OWN RE-READS.  256 x 256 tiles halve them:
// 8 wavefronts (4 x 2), each 64 x 128 of the tile (2 x 4 MFMA tiles, 128 accumulator registers), one workgroup per CU, 16-row stages
// of two fp16 planes per operand (74 KB), the same transpose reads on a 576-byte row pitch (= 16 banks mod 64 like the 320-byte one).
constexpr int WTD = 256, WTP = 288, WNT = 512;
__device__ __forceinline__ hwbf16x8 frag_trw(const bf16_t *p)      // frag_tr on the wide tile's row pitch
{
  typedef __attribute__((address_space(3))) v4s16 *lp;
  union { v4s16 h[2]; hwbf16x8 v; } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(p));
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(p + 4 * WTP));
  return u.v;
}

template <bool CONV>
__device__ __forceinline__ void wgrad_h2w_body(const float *__restrict__ dY, const float *__restrict__ X, float *__restrict__ dW,
                                               float *__restrict__ dB, float *__restrict__ ws, int M, int N, int K, int ldy, int ldx,
                                               int ldw, int tiles_k, int tiles, int m_chunk, int H, int W, int bid, int64_t ws_tile0,
                                               const float *__restrict__ y_amax, const float *__restrict__ x_amax)
{
  extern __shared__ __attribute__((aligned(16))) bf16_t Sw[];                // [stage 2][operand 2][plane 2][TWS][WTP]
  auto S = [&](int buf, int op, int pl, int r) -> bf16_t * { return Sw + ((((buf * 2 + op) * 2 + pl) * TWS + r) * WTP); };
  const int tile = bid % tiles, split = bid / tiles;
  const int n0 = (tile / tiles_k) * WTD, k0 = (tile % tiles_k) * WTD;
  const int mb = split * m_chunk, me = min(M, mb + m_chunk);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 128;
  const int sr = t >> 6, sc = (t & 63) * 4;                      // staging: rows sr, sr + 8; columns sc .. sc+3
  const bool ycol_ok = n0 + sc < N, xcol_ok = k0 + sc < K;
  float sy = 1.f, sx = 1.f, inv_yx = 1.f;
  if (y_amax || x_amax) {                                        // slab-wise power-of-two scales (see wgrad_tr_body)
    float my = 0.f, mx = 0.f;
    if (y_amax) for (int r = mb + t; r < me; r += WNT) my = fmaxf(my, y_amax[r]);
    const int xlo = CONV ? max(0, mb - W - 1) : mb, xhi = CONV ? min(M, me + W + 1) : me;
    if (x_amax) for (int r = xlo + t; r < xhi; r += WNT) mx = fmaxf(mx, x_amax[r]);
#pragma unroll
    for (int o = 32; o; o >>= 1) { my = fmaxf(my, __shfl_xor(my, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
    float *red = reinterpret_cast<float *>(Sw);
    if (lane == 0) { red[wave] = my; red[8 + wave] = mx; }
    __syncthreads();
    my = mx = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { my = fmaxf(my, red[i]); mx = fmaxf(mx, red[8 + i]); }
    __syncthreads();
    float iy = 1.f, ix = 1.f;
    if (y_amax) pdh2::row_scale(my, sy, iy);
    if (x_amax) pdh2::row_scale(mx, sx, ix);
    inv_yx = iy * ix;
  }
  float4 ry[2][2], rx[2][2];                                     // two register stages
  int cpy[2] = {0, 0}, cpx[2] = {0, 0}, tdy = 0, tdx = 0, xoff = k0 + sc;
  if (CONV) {
    const int tap = k0 / ldx;
    tdy = tap / 3 - 1; tdx = tap - (tap / 3) * 3 - 1;
    xoff = k0 - tap * ldx + sc;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int pix = (mb + sr + 8 * j) % (H * W);
      cpy[j] = pix / W; cpx[j] = pix - cpy[j] * W;
    }
  }
  auto gload = [&](int s, int m) {                               // called with m = mb, mb + 16, mb + 32, ... in this order
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = m + sr + 8 * j;
      ry[s][j] = (r < me && ycol_ok) ? *reinterpret_cast<const float4 *>(dY + (int64_t)r * ldy + n0 + sc) : make_float4(0, 0, 0, 0);
      if (CONV) {
        const int yy = cpy[j] + tdy, xx = cpx[j] + tdx;
        const bool ok = r < me && xcol_ok && yy >= 0 && yy < H && xx >= 0 && xx < W;
        rx[s][j] = ok ? *reinterpret_cast<const float4 *>(X + ((int64_t)r + tdy * W + tdx) * ldx + xoff) : make_float4(0, 0, 0, 0);
        cpx[j] += TWS;
        while (cpx[j] >= W) { cpx[j] -= W; if (++cpy[j] == H) cpy[j] = 0; }
      } else {
        rx[s][j] = (r < me && xcol_ok) ? *reinterpret_cast<const float4 *>(X + (int64_t)r * ldx + k0 + sc) : make_float4(0, 0, 0, 0);
      }
    }
  };
  const bool do_bias = dB != nullptr && k0 == 0;
  float4 bsum = make_float4(0, 0, 0, 0);
  auto lstore = [&](int s, int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = sr + 8 * j;
      const pdh2::SplitH y = pdh2::split4h(ry[s][j], sy), x = pdh2::split4h(rx[s][j], sx);
      *reinterpret_cast<uint2 *>(S(buf, 0, 0, r) + sc) = y.hi; *reinterpret_cast<uint2 *>(S(buf, 0, 1, r) + sc) = y.lo;
      *reinterpret_cast<uint2 *>(S(buf, 1, 0, r) + sc) = x.hi; *reinterpret_cast<uint2 *>(S(buf, 1, 1, r) + sc) = x.lo;
      if (do_bias) { bsum.x += ry[s][j].x; bsum.y += ry[s][j].y; bsum.z += ry[s][j].z; bsum.w += ry[s][j].w; }
    }
  };
  f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int steps = (me - mb + TWS - 1) / TWS;
  if (steps > 0) {
    gload(0, mb);
    if (steps > 1) gload(1, mb + TWS);
    lstore(0, 0);
  }
  __syncthreads();
  const int grp = lane >> 4, sl = lane & 15;
  const int frow = 8 * (grp >> 1) + (sl >> 2), fcol = 16 * (grp & 1) + 4 * (sl & 3);
  auto step = [&](int st, int par) {
    if (st + 2 < steps) gload(par, mb + (st + 2) * TWS);
    hwbf16x8 a[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int i = 0; i < 2; ++i) a[p][i] = frag_trw(S(par, 0, p, frow) + wn + i * 32 + fcol);
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {                             // two column tiles at a time (8, not 16, X fragments live)
      hwbf16x8 b[2][2];
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < 2; ++j) b[p][j] = frag_trw(S(par, 1, p, frow) + wk + (jp * 2 + j) * 32 + fcol);
#define WTERM(PA, PB)                                                        \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                              \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                          \
        pdh2::mmah(acc[i][jp * 2 + j], __builtin_bit_cast(pdh2::h16x8, a[PA][i]), __builtin_bit_cast(pdh2::h16x8, b[PB][j]));
      WTERM(1, 0) WTERM(0, 1) WTERM(0, 0)
#undef WTERM
    }
    if (st + 1 < steps) lstore(par ^ 1, par ^ 1);
    __syncthreads();
  };
  int st0 = 0;
  // Interior tiles (all 256 columns of both operands inside, whole 16-row stages): the same step as ONE basic block — no bounds
  // branches around the loads, the convolution's halo test a select on a load from the centre pixel's (always valid) address — with
  // the split, the LDS stores and the next loads laid between the matrix instructions (gemm_f16x2.hip's interleaved step).
  // The last two steps run through the guarded form.
  if (g_wgrad_fast && n0 + WTD <= N && k0 + WTD <= K && ((me - mb) % TWS) == 0 && steps >= 4 && (!CONV || W >= TWS)) {
    const float *py0 = dY + (int64_t)(mb + sr) * ldy + n0 + sc, *px0 = X + (int64_t)(mb + sr) * ldx + (CONV ? xoff : k0 + sc);
    auto fstep = [&](int st, int par) {
      const int64_t m = (int64_t)(st + 2) * TWS;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        ry[par][j] = *reinterpret_cast<const float4 *>(py0 + (m + 8 * j) * ldy);
        if (CONV) {
          const int yy = cpy[j] + tdy, xx = cpx[j] + tdx;
          const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
          const float4 v = *reinterpret_cast<const float4 *>(px0 + (m + 8 * j + (ok ? tdy * W + tdx : 0)) * ldx);
          rx[par][j] = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
          cpx[j] += TWS;
          const bool wrap = cpx[j] >= W;
          cpx[j] -= wrap ? W : 0;
          cpy[j] = wrap ? (cpy[j] + 1 == H ? 0 : cpy[j] + 1) : cpy[j];
        } else {
          rx[par][j] = *reinterpret_cast<const float4 *>(px0 + (m + 8 * j) * ldx);
        }
      }
      hwbf16x8 a[2][2], b[2][4];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int i = 0; i < 2; ++i) a[p][i] = frag_trw(S(par, 0, p, frow) + wn + i * 32 + fcol);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[p][j] = frag_trw(S(par, 1, p, frow) + wk + j * 32 + fcol);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = sr + 8 * j;
        const pdh2::SplitH y = pdh2::split4h(ry[par ^ 1][j], sy), x = pdh2::split4h(rx[par ^ 1][j], sx);
        *reinterpret_cast<uint2 *>(S(par ^ 1, 0, 0, r) + sc) = y.hi; *reinterpret_cast<uint2 *>(S(par ^ 1, 0, 1, r) + sc) = y.lo;
        *reinterpret_cast<uint2 *>(S(par ^ 1, 1, 0, r) + sc) = x.hi; *reinterpret_cast<uint2 *>(S(par ^ 1, 1, 1, r) + sc) = x.lo;
        bsum.x += ry[par ^ 1][j].x; bsum.y += ry[par ^ 1][j].y; bsum.z += ry[par ^ 1][j].z; bsum.w += ry[par ^ 1][j].w;   // read only when do_bias
      }
#define WFTERM(PA, PB)                                                       \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                              \
      _Pragma("unroll") for (int j = 0; j < 4; ++j)                          \
        pdh2::mmah(acc[i][j], __builtin_bit_cast(pdh2::h16x8, a[PA][i]), __builtin_bit_cast(pdh2::h16x8, b[PB][j]));
      WFTERM(1, 0) WFTERM(0, 1) WFTERM(0, 0)
#undef WFTERM
      __builtin_amdgcn_sched_group_barrier(0x100, 24, 0);
#pragma unroll
      for (int g = 0; g < 24; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        if (g % 3 == 2) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        if (g % 6 == 5) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
      __syncthreads();
    };
    for (; st0 + 3 < steps; st0 += 2) {
      fstep(st0, 0);
      fstep(st0 + 1, 1);
    }
  }
  for (int st = st0; st < steps; st += 2) {
    step(st, 0);
    if (st + 1 < steps) step(st + 1, 1);
  }
  if (do_bias) {
    float *red = reinterpret_cast<float *>(Sw);                  // the last step ended with a barrier: the stages are free
    *reinterpret_cast<float4 *>(red + sr * WTD + sc) = bsum;
    __syncthreads();
    if (t < WTD && n0 + t < N) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) v += red[r * WTD + t];
      unsafeAtomicAdd(dB + n0 + t, v);
    }
  }
  if (ws) {
    // partial tile in REGISTER order (element (ij, e) of thread t at ((ij * 16 + e) * 512 + t), ij = 4 i + j)
    float *w = ws + (ws_tile0 + (int64_t)split * tiles + tile) * (WTD * WTD) + t;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) w[((i * 4 + j) * 16 + e) * WNT] = acc[i][j][e] * inv_yx;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = k0 + wk + j * 32 + (lane & 31);
    if (c >= K) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = n0 + wn + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < N) unsafeAtomicAdd(dW + (int64_t)row * ldw + c, acc[i][j][e] * inv_yx);
      }
  }
}

template <bool CONV>
__global__ __launch_bounds__(512, 1) void gemm_wgrad_f16x2_wide(const float *__restrict__ dY, const float *__restrict__ X, float *__restrict__ dW,
                                                                float *__restrict__ dB, float *__restrict__ ws, int M, int N, int K, int ldy, int ldx,
                                                                int ldw, int tiles_k, int tiles, int m_chunk, int H, int W,
                                                                const float *__restrict__ y_amax, const float *__restrict__ x_amax)
{
  wgrad_h2w_body<CONV>(dY, X, dW, dB, ws, M, N, K, ldy, ldx, ldw, tiles_k, tiles, m_chunk, H, W, xcd_chunk((int)blockIdx.x, (int)gridDim.x), 0,
                       y_amax, x_amax);
}

// element (q = ij * 16 + e, thread t) of a wide partial tile -> (output row, column) of the tile
__device__ __forceinline__ void h2w_coord(int q, int t, int &row, int &col)
{
  const int lane = t & 63, wave = t >> 6, ij = q >> 4, e = q & 15, i = ij >> 2, j = ij & 3;
  row = (wave >> 1) * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
  col = (wave & 1) * 128 + j * 32 + (lane & 31);
}

// dW tile += sum over splits of the partial tiles (128 blocks of 512 threads per tile, one (ij, e) each; blockIdx.y takes every
// gridDim.y-th split and finishes with an atomic, gridDim.y == 1 owns its element)
__global__ __launch_bounds__(512) void wgrad_h2w_reduce(const float *__restrict__ ws, float *__restrict__ dW, int N, int K, int ldw, int tiles_k,
                                                        int tiles, int splits)
{
  const int tile = blockIdx.x >> 7, q = blockIdx.x & 127, t = threadIdx.x;
  const int n0 = (tile / tiles_k) * WTD, k0 = (tile % tiles_k) * WTD;
  const float *p = ws + (int64_t)tile * (WTD * WTD) + q * WNT + t;
  const int64_t stride = (int64_t)tiles * (WTD * WTD);
  float s0 = 0.f, s1 = 0.f;
  int sp = blockIdx.y;
  const int G = gridDim.y;
  for (; sp + 7 * G < splits; sp += 8 * G) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(sp + u * G) * stride];
#pragma unroll
    for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
  }
  for (; sp < splits; sp += G) s0 += p[(int64_t)sp * stride];
  int row, col;
  h2w_coord(q, t, row, col);
  if (k0 + col < K && n0 + row < N) {
    float *d = dW + (int64_t)(n0 + row) * ldw + k0 + col;
    if (G == 1) *d += s0 + s1; else unsafeAtomicAdd(d, s0 + s1);
  }
}

// Several weight gradients in ONE launch (pd_gemm_wgrad_f32x3_grouped): a table of problems in device memory, workgroup b belongs
// to the problem whose [block0, block0 + tiles * splits) contains b.  The encoder's 30 weight gradients per step are independent of
// everything until the optimizer runs, so they are queued during its backward pass and run here together: every (tile, split)
// workgroup of the launch walks the same number of rows, the machine is filled in whole rounds once instead of 30 times, and
// the partial-tile traffic falls from 512 tiles per GEMM to ~17 splits per output tile.
struct WgradX3Problem {
  const float *dY, *X;
  float *dW, *dB;
  int M, N, K, ldy, ldx, ldw, tiles_k, tiles, m_chunk, splits, block0, pad;
  int64_t ws_tile0;
  const float *y_amax, *x_amax;
};

template <bool H2>
__global__ __launch_bounds__(256, 2) void gemm_wgrad_f32x3_tr_grouped(const WgradX3Problem *__restrict__ tab, int count, float *__restrict__ ws)
{
  const int lb = g_wgrad_xcd ? xcd_chunk((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;     // see gemm_wgrad_f32x3_tr
  int p = 0;
  while (p + 1 < count && lb >= tab[p + 1].block0) ++p;                   // <= a few dozen problems: a scalar scan
  const WgradX3Problem q = tab[p];
  wgrad_tr_body<0, false, H2>(pd_as_global(q.dY), pd_as_global(q.X), pd_as_global(q.dW), pd_as_global(q.dB), ws, q.M, q.N, q.K, q.ldy, q.ldx, q.ldw, q.tiles_k, q.tiles, q.m_chunk, 0, 0,
                              lb - q.block0, q.ws_tile0, pd_as_global(q.y_amax), pd_as_global(q.x_amax));   // (pd_common.h: table pointers would be FLAT)
}

// grouped form of wgrad_tr_reduce: blockIdx.x = 64 x (global output tile index); the problem is found from its first tile
__global__ __launch_bounds__(256) void wgrad_tr_reduce_grouped(const WgradX3Problem *__restrict__ tab, int count, const float *__restrict__ ws)
{
  const int gt = blockIdx.x >> 6, q = blockIdx.x & 63;
  int p = 0, t0 = 0;
  while (p + 1 < count && gt >= t0 + tab[p].tiles) { t0 += tab[p].tiles; ++p; }
  const WgradX3Problem pr = tab[p];
  const int tile = gt - t0;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ij = q >> 4, e = q & 15, i = ij >> 1, j = ij & 1;
  const int n0 = (tile / pr.tiles_k) * BN, k0 = (tile % pr.tiles_k) * BM;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;
  const float *src = ws + (pr.ws_tile0 + tile) * (BN * BM) + q * 256 + t;
  const int64_t stride = (int64_t)pr.tiles * (BN * BM);
  float s0 = 0.f, s1 = 0.f;
  int sp = 0;
  for (; sp + 7 < pr.splits; sp += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(sp + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
  }
  for (; sp < pr.splits; ++sp) s0 += src[(int64_t)sp * stride];
  const int c = k0 + wk + j * 32 + (lane & 31);
  const int row = n0 + wn + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
  if (c < pr.K && row < pr.N) pd_as_global(pr.dW)[(int64_t)row * pr.ldw + c] += s0 + s1;      // this block owns the element: plain read-modify-write
}

__global__ __launch_bounds__(512, 1) void gemm_wgrad_f16x2_wide_grouped(const WgradX3Problem *__restrict__ tab, int count, float *__restrict__ ws)
{
  const int lb = xcd_chunk((int)blockIdx.x, (int)gridDim.x);
  int p = 0;
  while (p + 1 < count && lb >= tab[p + 1].block0) ++p;
  const WgradX3Problem q = tab[p];
  wgrad_h2w_body<false>(pd_as_global(q.dY), pd_as_global(q.X), pd_as_global(q.dW), pd_as_global(q.dB), ws, q.M, q.N, q.K, q.ldy, q.ldx, q.ldw, q.tiles_k, q.tiles, q.m_chunk, 0, 0, lb - q.block0, q.ws_tile0,
                        pd_as_global(q.y_amax), pd_as_global(q.x_amax));
}

__global__ __launch_bounds__(512) void wgrad_h2w_reduce_grouped(const WgradX3Problem *__restrict__ tab, int count, const float *__restrict__ ws)
{
  const int gt = blockIdx.x >> 7, q = blockIdx.x & 127, t = threadIdx.x;
  int p = 0, t0 = 0;
  while (p + 1 < count && gt >= t0 + tab[p].tiles) { t0 += tab[p].tiles; ++p; }
  const WgradX3Problem pr = tab[p];
  const int tile = gt - t0;
  const int n0 = (tile / pr.tiles_k) * WTD, k0 = (tile % pr.tiles_k) * WTD;
  const float *src = ws + (pr.ws_tile0 + tile) * (WTD * WTD) + q * WNT + t;
  const int64_t stride = (int64_t)pr.tiles * (WTD * WTD);
  float s0 = 0.f, s1 = 0.f;
  int sp = 0;
  for (; sp + 7 < pr.splits; sp += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(sp + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
  }
  for (; sp < pr.splits; ++sp) s0 += src[(int64_t)sp * stride];
  int row, col;
  h2w_coord(q, t, row, col);
  if (k0 + col < pr.K && n0 + row < pr.N) pd_as_global(pr.dW)[(int64_t)(n0 + row) * pr.ldw + k0 + col] += s0 + s1;
}

// dW tile += sum over splits of the partial tiles gemm_wgrad_f32x3_tr left in the workspace (same register-order indexing)
__global__ __launch_bounds__(256) void wgrad_tr_reduce(const float *__restrict__ ws, float *__restrict__ dW, int N, int K, int ldw, int tiles_k,
                                                       int tiles, int splits)
{
  const int tile = blockIdx.x >> 6, q = blockIdx.x & 63;         // 64 blocks per tile, one (ij, e) each
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ij = q >> 4, e = q & 15, i = ij >> 1, j = ij & 1;
  const int n0 = (tile / tiles_k) * BN, k0 = (tile % tiles_k) * BM;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;
  // blockIdx.y takes every gridDim.y-th split: 8 independent loads in flight per thread, a few atomics per element at the end
  const float *p = ws + (int64_t)tile * (BN * BM) + q * 256 + t;
  const int64_t stride = (int64_t)tiles * (BN * BM);
  float s0 = 0.f, s1 = 0.f;
  int sp = blockIdx.y;
  const int G = gridDim.y;
  for (; sp + 7 * G < splits; sp += 8 * G) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(sp + u * G) * stride];
#pragma unroll
    for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
  }
  for (; sp < splits; sp += G) s0 += p[(int64_t)sp * stride];
  const int c = k0 + wk + j * 32 + (lane & 31);
  const int row = n0 + wn + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
  if (c < K && row < N) unsafeAtomicAdd(dW + (int64_t)row * ldw + c, s0 + s1);
}
}  // namespace

extern "C" void pd_dbg_set_wgrad_xcd(int v) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wgrad_xcd), &v, sizeof(int)); }
extern "C" void pd_dbg_set_wgrad_fast(int v) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wgrad_fast), &v, sizeof(int)); }
int g_pd_dbg_wgrad_wide = 1;   // tools only (pd_debug_set "wgrad_wide" 0: the 128 x 128 kernel for every f16x2 weight gradient)
// the f16x2 weight gradient takes 256 x 256 tiles when the output has several of them (measured at M = 43 008, tools/bench_wgrad_x3.py:
// 1024 x 256 104 vs 126 us, 256 x 2304 195 vs 257; a single 256 x 256 tile LOSES, 48 vs 42 us — 256 slices of rows each leave a 256 KB
// partial tile) and, for the 3 x 3 convolution, a tile's 256 X columns lie inside one tap
static bool wgrad_wide_ok(int N, int K, int conv_ci)
{
  return g_pd_dbg_wgrad_wide && N > 128 && K > 128 && (N >= 1024 || K >= 1024) && (conv_ci == 0 || conv_ci % WTD == 0);
}
extern "C" int pd_gemm_wgrad_f16x2_takes_wide_tiles(int N, int K) { return wgrad_wide_ok(N, K, 0) ? 1 : 0; }

static int wgrad_x3_launch(const float *dY, const float *X, float *dW, float *dB, float *ws, int64_t ws_floats, int M, int N, int K, int ldy,
                           int ldx, int ldw, hipStream_t st, const char *who, int convH = 0, int convW = 0, bool h2 = false,
                           const float *y_amax = nullptr, const float *x_amax = nullptr)
{
  if (M < 0 || N < 0 || K < 0) return pd_set_error(PD_ERR_INVALID_ARG, "%s: negative size", who);
  if (N == 0 || K == 0 || M == 0) return PD_OK;
  if (!dW || !dY || !X) return pd_set_error(PD_ERR_INVALID_ARG, "%s: null pointer", who);
  const int tk = (K + BM - 1) / BM, tn = (N + BN - 1) / BN, tiles = tk * tn;
  // the contraction is split over workgroups (each ends in a tile of atomics, or of plain stores into the workspace).  Two
  // workgroups are resident per CU, so the launch is sized to ONE round of 512: 1 044 workgroups (the old "~4 per CU" rule at
  // 256 x 2304) ran as 3 rounds, the last one almost empty — 387 us instead of 260.
  int splits = tiles >= 512 ? 1 : (512 + tiles / 2) / tiles;
  int m_chunk = ((M + splits - 1) / splits + WS - 1) / WS * WS;
  if (m_chunk < 4 * WS) m_chunk = 4 * WS;
  splits = (M + m_chunk - 1) / m_chunk;
  // transpose-read form when the operands allow 16-byte row loads (always, in this repo)
  const bool vec = !(N & 3) && !(K & 3) && !(ldy & 3) && !(ldx & 3) && !((uintptr_t)dY & 15) && !((uintptr_t)X & 15);
  if (convH && !vec) return pd_set_error(PD_ERR_INVALID_ARG, "%s: channel counts must be multiples of 4 and the tensors 16-byte aligned", who);
  if (h2 && !vec) return pd_set_error(PD_ERR_INVALID_ARG, "%s: N, K, ldy, ldx must be multiples of 4 and dY, X 16-byte aligned", who);
  if (!vec) {
    hipLaunchKernelGGL(gemm_wgrad_f32x3, dim3((unsigned)(tiles * splits)), dim3(256), 0, st, dY, X, dW, dB, M, N, K, ldy, ldx, ldw, tk, tiles,
                       m_chunk);
    return pd_check_launch(who);
  }
  if (h2 && wgrad_wide_ok(N, K, convH ? ldx : 0)) {
    // 256 x 256 tiles, one workgroup per CU: one round of 256
    const int wtk = (K + WTD - 1) / WTD, wtn = (N + WTD - 1) / WTD, wtiles = wtk * wtn;
    int wsplits = wtiles >= 256 ? 1 : (256 + wtiles / 2) / wtiles;
    int mc = ((M + wsplits - 1) / wsplits + TWS - 1) / TWS * TWS;
    if (mc < 4 * TWS) mc = 4 * TWS;
    wsplits = (M + mc - 1) / mc;
    if (ws && (ws_floats < (int64_t)wtiles * wsplits * WTD * WTD || wsplits < 2)) ws = nullptr;
    constexpr size_t lds = (size_t)2 * 2 * 2 * TWS * WTP * sizeof(bf16_t);
    static bool attr = false;
    if (!attr) {
      (void)hipFuncSetAttribute((const void *)gemm_wgrad_f16x2_wide<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      (void)hipFuncSetAttribute((const void *)gemm_wgrad_f16x2_wide<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      attr = true;
    }
    auto kw = convH ? gemm_wgrad_f16x2_wide<true> : gemm_wgrad_f16x2_wide<false>;
    hipLaunchKernelGGL(kw, dim3((unsigned)(wtiles * wsplits)), dim3(WNT), lds, st, dY, X, dW, dB, ws, M, N, K, ldy, ldx, ldw, wtk, wtiles, mc, convH, convW,
                       y_amax, x_amax);
    const int wgroups = wtiles * 128 >= 2048 ? 1 : wsplits >= 64 ? 8 : wsplits >= 16 ? 4 : 1;
    if (ws) hipLaunchKernelGGL(wgrad_h2w_reduce, dim3((unsigned)(wtiles * 128), wgroups), dim3(WNT), 0, st, (const float *)ws, dW, N, K, ldw, wtk, wtiles, wsplits);
    return pd_check_launch(who);
  }
  if (ws && (ws_floats < (int64_t)tiles * splits * BN * BM || splits < 2)) ws = nullptr;   // not worth / does not fit: atomics
  auto kfn = h2 ? (convH ? gemm_wgrad_f32x3_tr<0, true, true> : gemm_wgrad_f32x3_tr<0, false, true>)
                 : gemm_wgrad_f32x3_tr<0, false>;                 // (a convolution always comes in the two-plane form)
  hipLaunchKernelGGL(kfn, dim3((unsigned)(tiles * splits)), dim3(256), 0, st, dY, X, dW, dB, ws, M, N, K, ldy, ldx, ldw, tk, tiles, m_chunk,
                     convH, convW, y_amax, x_amax);
  const int groups = tiles * 64 >= 2048 ? 1 : splits >= 64 ? 8 : splits >= 16 ? 4 : 1;
  if (ws) hipLaunchKernelGGL(wgrad_tr_reduce, dim3((unsigned)(tiles * 64), groups), dim3(256), 0, st, (const float *)ws, dW, N, K, ldw, tk, tiles,
                             splits);
  return pd_check_launch(who);
}


// ---- grouped weight gradients (include/pd_gemm.h: pd_gemm_wgrad_f32x3_grouped)
extern "C" int64_t pd_gemm_wgrad_f32x3_grouped_table_bytes(int max_count) { return (int64_t)(max_count > 0 ? max_count : 0) * (int64_t)sizeof(WgradX3Problem); }

static bool grouped_wide(const PdGemmWgradDesc *d, int count)
{
  for (int i = 0; i < count; ++i) if (!wgrad_wide_ok(d[i].N, d[i].K, 0)) return false;
  return count > 0;
}

// TD: tile edge (128, or 256 for the wide f16x2 kernel: one workgroup per CU, rounds of 256)
static int grouped_plan(const PdGemmWgradDesc *d, int count, WgradX3Problem *tab, int64_t *ws_tiles, int *blocks, int TD = BM)
{
  int64_t total_tiles = 0;
  for (int i = 0; i < count; ++i) {
    if (d[i].M <= 0 || d[i].N <= 0 || d[i].K <= 0 || !d[i].dY || !d[i].X || !d[i].dW) return 1;
    if ((d[i].N & 3) || (d[i].K & 3) || (d[i].ldy & 3) || (d[i].ldx & 3) || ((uintptr_t)d[i].dY & 15) || ((uintptr_t)d[i].X & 15)) return 1;
    total_tiles += (int64_t)((d[i].K + TD - 1) / TD) * ((d[i].N + TD - 1) / TD);
  }
  // one split count for all problems, chosen so that the launch is a whole number of rounds of 512 resident workgroups (two per
  // CU): tiles x splits just below a multiple of 512, at least ~6 rounds deep so that unequal M do not leave a ragged tail
  int splits = (int)((6 * (TD == BM ? 512 : 256)) / (total_tiles > 0 ? total_tiles : 1));
  if (splits < 1) splits = 1;
  int64_t wt = 0; int b0 = 0;
  for (int i = 0; i < count; ++i) {
    WgradX3Problem &q = tab[i];
    q.dY = d[i].dY; q.X = d[i].X; q.dW = d[i].dW; q.dB = d[i].dB;
    q.M = d[i].M; q.N = d[i].N; q.K = d[i].K; q.ldy = d[i].ldy; q.ldx = d[i].ldx; q.ldw = d[i].ldw;
    q.tiles_k = (q.K + TD - 1) / TD; q.tiles = q.tiles_k * ((q.N + TD - 1) / TD);
    int mc = ((q.M + splits - 1) / splits + TWS - 1) / TWS * TWS;
    if (mc < 4 * TWS) mc = 4 * TWS;
    q.m_chunk = mc; q.splits = (q.M + mc - 1) / mc;
    q.block0 = b0; q.pad = 0; q.ws_tile0 = wt;
    q.y_amax = d[i].y_amax; q.x_amax = d[i].x_amax;
    b0 += q.tiles * q.splits; wt += (int64_t)q.tiles * q.splits;
  }
  *ws_tiles = wt; *blocks = b0;
  return 0;
}

extern "C" int64_t pd_gemm_wgrad_f32x3_grouped_ws_floats(const PdGemmWgradDesc *descs, int count)
{
  if (count <= 0 || count > 256 || !descs) return 0;
  WgradX3Problem tab[256];
  int64_t wt = 0; int blocks = 0;
  if (grouped_plan(descs, count, tab, &wt, &blocks)) return -1;
  return wt * BN * BM;
}

static int wgrad_grouped(const PdGemmWgradDesc *descs, int count, void *table_host_pinned, void *table_device, float *workspace,
                         int64_t workspace_floats, void *stream_, bool h2)
{
  if (count == 0) return PD_OK;
  if (count < 0 || count > 256 || !descs || !table_host_pinned || !table_device || !workspace)
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_gemm_wgrad_f32x3_grouped: count=%d (1..256) or null pointer", count);
  WgradX3Problem *tab = reinterpret_cast<WgradX3Problem *>(table_host_pinned);
  int64_t wt = 0; int blocks = 0;
  const bool wide = h2 && grouped_wide(descs, count);
  const int TD = wide ? WTD : BM;
  if (grouped_plan(descs, count, tab, &wt, &blocks, TD))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_gemm_wgrad_f32x3_grouped: every problem needs M, N, K > 0, N, K, ldy, ldx multiples of 4, 16-byte aligned operands");
  if (workspace_floats < wt * TD * TD) return pd_set_error(PD_ERR_INVALID_ARG, "pd_gemm_wgrad_f32x3_grouped: workspace too small");
  hipStream_t st = (hipStream_t)stream_;
  if (hipMemcpyAsync(table_device, table_host_pinned, (size_t)count * sizeof(WgradX3Problem), hipMemcpyHostToDevice, st) != hipSuccess)
    return pd_set_error(PD_ERR_LAUNCH, "pd_gemm_wgrad_f32x3_grouped: table upload failed");
  const WgradX3Problem *dt = reinterpret_cast<const WgradX3Problem *>(table_device);
  int64_t tiles = 0;
  for (int i = 0; i < count; ++i) tiles += tab[i].tiles;
  if (wide) {
    constexpr size_t lds = (size_t)2 * 2 * 2 * TWS * WTP * sizeof(bf16_t);
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void *)gemm_wgrad_f16x2_wide_grouped, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr = true; }
    hipLaunchKernelGGL(gemm_wgrad_f16x2_wide_grouped, dim3((unsigned)blocks), dim3(WNT), lds, st, dt, count, workspace);
    hipLaunchKernelGGL(wgrad_h2w_reduce_grouped, dim3((unsigned)(tiles * 128)), dim3(WNT), 0, st, dt, count, (const float *)workspace);
    return pd_check_launch("pd_gemm_wgrad_f16x2_grouped");
  }
  if (h2) hipLaunchKernelGGL(gemm_wgrad_f32x3_tr_grouped<true>, dim3((unsigned)blocks), dim3(256), 0, st, dt, count, workspace);
  else hipLaunchKernelGGL(gemm_wgrad_f32x3_tr_grouped<false>, dim3((unsigned)blocks), dim3(256), 0, st, dt, count, workspace);
  hipLaunchKernelGGL(wgrad_tr_reduce_grouped, dim3((unsigned)(tiles * 64)), dim3(256), 0, st, dt, count, (const float *)workspace);
  return pd_check_launch("pd_gemm_wgrad_f32x3_grouped");
}

extern "C" int pd_gemm_wgrad_f32x3_grouped(const PdGemmWgradDesc *descs, int count, void *table_host_pinned, void *table_device,
                                           float *workspace, int64_t workspace_floats, void *stream_)
{
  return wgrad_grouped(descs, count, table_host_pinned, table_device, workspace, workspace_floats, stream_, false);
}

extern "C" int pd_gemm_wgrad_f16x2_grouped(const PdGemmWgradDesc *descs, int count, void *table_host_pinned, void *table_device,
                                           float *workspace, int64_t workspace_floats, void *stream_)
{
  return wgrad_grouped(descs, count, table_host_pinned, table_device, workspace, workspace_floats, stream_, true);
}

extern "C" int64_t pd_gemm_wgrad_f16x2_ws_floats(int N, int K)
{
  const int64_t narrow = pd_gemm_wgrad_f32x3_ws_floats(N, K);
  if (N <= 0 || K <= 0) return narrow;
  const int64_t wt = (int64_t)((K + WTD - 1) / WTD) * ((N + WTD - 1) / WTD);
  const int64_t wide = wt >= 256 ? 0 : (256 + wt / 2) / wt * wt * WTD * WTD;
  return wide > narrow ? wide : narrow;                          // whichever tile shape the launch takes
}

extern "C" int64_t pd_gemm_wgrad_f16x2_grouped_ws_floats(const PdGemmWgradDesc *descs, int count)
{
  if (count <= 0 || count > 256 || !descs) return 0;
  WgradX3Problem tab[256];
  int64_t wt = 0; int blocks = 0;
  const int TD = grouped_wide(descs, count) ? WTD : BM;
  if (grouped_plan(descs, count, tab, &wt, &blocks, TD)) return -1;
  return wt * TD * TD;
}

extern "C" int pd_gemm_wgrad_acc_f16x2_ws(const float *dY, const float *X, float *dW, float *dB, const float *y_amax, const float *x_amax,
                                          float *workspace, int64_t workspace_floats, int M, int N, int K, int ldy, int ldx, int ldw, void *stream_)
{
  return wgrad_x3_launch(dY, X, dW, dB, workspace, workspace_floats, M, N, K, ldy, ldx, ldw, (hipStream_t)stream_, "pd_gemm_wgrad_acc_f16x2_ws", 0, 0,
                         true, y_amax, x_amax);
}

extern "C" int pd_conv3x3_wgrad_nhwc_f16x2(const float *dY, const float *X, float *dWk, float *dB, const float *y_amax, const float *x_amax,
                                           float *workspace, int64_t workspace_floats, int B, int H, int W, int Ci, int Co, void *stream_)
{
  if (B < 0 || H <= 0 || W <= 0 || Ci <= 0 || Co <= 0 || (Ci % BM) || (Co & 3))
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv3x3_wgrad_nhwc_f16x2: B=%d H=%d W=%d Ci=%d (%% 128) Co=%d (%% 4)", B, H, W, Ci, Co);
  const int64_t M = (int64_t)B * H * W;
  if (M > 0x7fffffffLL - 4096) return pd_set_error(PD_ERR_INVALID_ARG, "pd_conv3x3_wgrad_nhwc_f16x2: too many pixels");
  return wgrad_x3_launch(dY, X, dWk, dB, workspace, workspace_floats, (int)M, Co, 9 * Ci, Co, Ci, 9 * Ci, (hipStream_t)stream_,
                         "pd_conv3x3_wgrad_nhwc_f16x2", H, W, true, y_amax, x_amax);
}

extern "C" int pd_gemm_wgrad_acc_f32x3(const float *dY, const float *X, float *dW, float *dB, int M, int N, int K, int ldy, int ldx,
                                       int ldw, void *stream_)
{
  return wgrad_x3_launch(dY, X, dW, dB, nullptr, 0, M, N, K, ldy, ldx, ldw, (hipStream_t)stream_, "pd_gemm_wgrad_acc_f32x3");
}

extern "C" int64_t pd_gemm_wgrad_f32x3_ws_floats(int N, int K)
{
  const int64_t tiles = (int64_t)((K + BM - 1) / BM) * ((N + BN - 1) / BN);
  return tiles >= 512 ? 0 : (512 + tiles / 2) / tiles * tiles * BN * BM;     // <= 8.5 M floats (34 MB) whatever the shape
}

extern "C" int pd_gemm_wgrad_acc_f32x3_ws(const float *dY, const float *X, float *dW, float *dB, float *workspace, int64_t workspace_floats,
                                          int M, int N, int K, int ldy, int ldx, int ldw, void *stream_)
{
  return wgrad_x3_launch(dY, X, dW, dB, workspace, workspace_floats, M, N, K, ldy, ldx, ldw, (hipStream_t)stream_, "pd_gemm_wgrad_acc_f32x3_ws");
}
