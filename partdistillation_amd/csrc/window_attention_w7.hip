// Swin (shifted-)window attention for gfx950: 7 x 7 windows (49 tokens, Swin-T / Swin-S), head_dim 32, bf16 on
// v_mfma_f32_16x16x16_bf16_1k, fp32 softmax.  C-ABI and the math it replaces: include/pd_window_attention.h.  The 12 x 12 kernels
// (window_attention.hip) are the model: same MFMA operand convention, same LDS row image (64-byte rows, 16-byte chunks XOR-swizzled so
// that the 8-byte operand reads and the transposing reads are conflict-free), same phases in the backward.  What differs:
//
// * 49 tokens are padded to 64 on chip: one WORKGROUP of 4 wavefronts owns one (window, head) at a time, wave w the w-th 16-row tile
//   (rows 48..63 of wave 3 hold one real token).  Rows 49..63 of every LDS tile are ZEROED ONCE per workgroup and never written again, so a
//   transposed operand (V^T, dO^T, Q^T, K^T) is 0 there and 0 * 0 is what the MFMA adds for a padded row.  Padded KEYS get score -inf in the
//   forward and probability 0 (a select, not a product) in the backward — never the mask's -100; padded QUERIES are computed with
//   the whole wave active (ds_read_b64_tr_b16 needs EXEC all ones) and not stored; their probabilities are selected to 0 in the backward so
//   dK, dV and the table gradient get nothing from them.
// * Tiles are staged through registers (global load at the top of a window, LDS store after its arithmetic, one barrier per window): the
//   direct global -> LDS load of the 12 x 12 kernels writes whole 1 KiB blocks per wave and cannot leave the padded rows alone.  The O
//   tile never reaches LDS: delta = rowsum(dO * O) is formed from the staging registers.
// * A window row is 7 tokens, so the 4 keys a lane holds do not have consecutive table entries: the index A(q) - A(key) + 84,
//   A(t) = t + 6 * (t / 7), is computed per element (t clamped to 48 for padded tokens: the address stays inside the table).
// * A (window, head) unit is ~8.6 x less work than at window 12; the workgroup walks `chunk` (<= 16) windows of one head so the table staging
//   and, in the backward, the table-gradient reduction + 169 atomics are paid once per chunk (DESIGN.md has the measured alternative).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_bf16.h"
#include "pd_common.h"
#include "pd_msda.h"
#include "pd_window_attention.h"

extern int g_pd_dbg_wattn_chunk;   // pd_debug_set "wattn_chunk" (window_attention.hip): 1..8 forces that many windows per workgroup, 0 = chunk_of

namespace {
using namespace pdmfma;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int N = 49, NP = 64, D = 32, NT = 4, TBL = 169, THREADS = 64 * NT, MAX_CHUNK = 16;
constexpr int TILE_B = NP * 64;                                  // bytes of one [64][32] bf16 tile
constexpr float LOG2E = 1.4426950408889634f;
constexpr float MASKED = -100.0f * LOG2E;    // the reference's additive -100 in base-2 units

__device__ __forceinline__ void mma16(f32x4 &c, bf16x4 x, bf16x4 y) { c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(x, y, c, 0, 0, 0); }
// A(t) = t + 6 * (t / 7) = 13 * row + col of token t; padded tokens (49..63) take the last token's value so that every index stays in [0, 168]
__device__ __forceinline__ int rel_a(int t) { t = t < N - 1 ? t : N - 1; return t + 6 * ((t * 37) >> 8); }
__device__ __forceinline__ void st4(bf16_t *p, float a, float b, float c, float d) { *reinterpret_cast<bf16x4 *>(p) = pack4(a, b, c, d); }
__device__ __forceinline__ bf16x4 rd8(const unsigned char *p) { return *reinterpret_cast<const bf16x4 *>(p); }
__device__ __forceinline__ bf16x4 rdtr(const unsigned char *p)
{
  typedef __attribute__((address_space(3))) bf16x4 *lp;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)p);
}
// LDS image of a tile (as window_attention.hip): row r = 64 bytes, its 16-byte chunk ch at slot ch ^ swz(r)
__device__ __forceinline__ int swz(int row) { return ((row >> 3) & 1) | (((row >> 2) & 1) << 1); }
// byte offset inside a 16-row block of the 8-byte piece p (elements 4 p .. 4 p + 3) of row `row` (0..15)
__device__ __forceinline__ int piece_at(int row, int p) { return row * 64 + ((((p >> 1) ^ swz(row)) & 3) << 4) + ((p & 1) << 3); }
__device__ __forceinline__ float dot8(const uint4 &a, const uint4 &o)
{
  return bf_lo(a.x) * bf_lo(o.x) + bf_hi(a.x) * bf_hi(o.x) + bf_lo(a.y) * bf_lo(o.y) + bf_hi(a.y) * bf_hi(o.y)
       + bf_lo(a.z) * bf_lo(o.z) + bf_hi(a.z) * bf_hi(o.z) + bf_lo(a.w) * bf_lo(o.w) + bf_hi(a.w) * bf_hi(o.w);
}

template <bool MASK>
__global__ __launch_bounds__(THREADS) void wattn7_fwd(const bf16_t *__restrict__ qkv, const float *__restrict__ table,
                                                      const uint8_t *__restrict__ region, const uint8_t *__restrict__ flags,
                                                      bf16_t *__restrict__ out, float *__restrict__ lse, int B_, int nW,
                                                      int heads, float c1, int chunk)
{
  __shared__ __attribute__((aligned(16))) unsigned char kv[2 * 2 * TILE_B];     // [buffer][K, V]
  __shared__ __attribute__((aligned(16))) unsigned char reg_all[2 * NP];        // [buffer][token]
  __shared__ float tbl[TBL];
  const int tid = threadIdx.x, lane = tid & 63, qt = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 15, g = lane >> 4, h = blockIdx.y;
  const int C = heads * D;
  const int64_t ld = 3 * C;
  // staging: thread tid moves the 16 bytes of LDS slot tid & 3 of row tid / 4 of each tile
  const int lrow = tid >> 2, lch = (tid & 3) ^ swz(lrow);
  const bool lrow_ok = lrow < N;
  const int q = 16 * qt + c;
  const bool q_ok = q < N;
  const int b0 = blockIdx.x * chunk, n_units = min(chunk, B_ - b0);
  uint4 kn = {0u, 0u, 0u, 0u}, vn = kn;
  bf16x4 qn0 = {0, 0, 0, 0}, qn1 = qn0;                                   // this wave's query rows as MFMA operands, straight from memory (0 for padded rows)
  unsigned rn = 0;
  auto fetch = [&](int b) {
    if (lrow_ok) {
      const bf16_t *base = qkv + ((int64_t)b * N + lrow) * ld + h * D + lch * 8;
      kn = *reinterpret_cast<const uint4 *>(base + C);
      vn = *reinterpret_cast<const uint4 *>(base + 2 * C);
    }
    if (q_ok) {
      const bf16_t *qb = qkv + ((int64_t)b * N + q) * ld + h * D;
      qn0 = *reinterpret_cast<const bf16x4 *>(qb + 4 * g); qn1 = *reinterpret_cast<const bf16x4 *>(qb + 16 + 4 * g);
    }
    if (MASK && tid < N) rn = region[(int64_t)(b % nW) * N + tid];
  };
  auto stash = [&](int buf) {
    if (lrow_ok) {
      *reinterpret_cast<uint4 *>(kv + buf * 2 * TILE_B + tid * 16) = kn;
      *reinterpret_cast<uint4 *>(kv + buf * 2 * TILE_B + TILE_B + tid * 16) = vn;
    }
    if (MASK && tid < N) reg_all[buf * NP + tid] = (unsigned char)rn;
  };
  fetch(b0);
  if (!lrow_ok) {                                                         // the padded rows of all four tiles: zero, once
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<uint4 *>(kv + t * TILE_B + tid * 16) = uint4{0u, 0u, 0u, 0u};
  }
  if (tid >= N && tid < NP) reg_all[tid] = reg_all[NP + tid] = 0;
  unsigned long long mbits = 0;                                           // which of this workgroup's windows carry a mask (chunk <= 16)
  if (MASK) mbits = __ballot(lane < n_units && flags[(b0 + (lane < n_units ? lane : 0)) % nW] != 0);
  for (int i = tid; i < TBL; i += THREADS) tbl[i] = table[i * heads + h] * LOG2E;
  stash(0);

  const int off0 = piece_at(c, g), off1 = piece_at(c, 4 + g), toff0 = piece_at(4 * g + (c >> 2), c & 3), toff1 = piece_at(4 * g + (c >> 2), 4 + (c & 3));
  const int aq = rel_a(q) + 84;
  for (int u = 0; u < n_units; ++u) {
    const int b = b0 + u, buf = u & 1;
    const unsigned char *ks = kv + buf * 2 * TILE_B, *vs = ks + TILE_B, *r = reg_all + buf * NP;
    __syncthreads();                                                      // window u is in LDS; window u - 1 is done with
    const bf16x4 q0 = qn0, q1 = qn1;
    if (u + 1 < n_units) fetch(b + 1);
    const bool masked = MASK && ((mbits >> u) & 1);
    const unsigned rq = masked ? r[q] : 0u;
    f32x4 s[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      mma16(s[kt], rd8(ks + kt * 1024 + off0), q0);                       // S^T[key = 4g+e][q = c]
      mma16(s[kt], rd8(ks + kt * 1024 + off1), q1);
    }
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      unsigned rk = 0;
      if (masked) rk = *reinterpret_cast<const unsigned *>(r + 16 * kt + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int key = 16 * kt + 4 * g + e;
        float t = fmaf(s[kt][e], c1, tbl[aq - rel_a(key)]);
        if (masked && ((rk >> (8 * e)) & 255u) != rq) t += MASKED;
        if (key >= N) t = -INFINITY;                                      // a padded key: weight exactly 0
        s[kt][e] = t;
        m = fmaxf(m, t);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    float sum = 0.f;
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { s[kt][e] = __builtin_amdgcn_exp2f(s[kt][e] - m); sum += s[kt][e]; }
      const bf16x4 p = pack4(s[kt][0], s[kt][1], s[kt][2], s[kt][3]);
      mma16(o0, rdtr(vs + kt * 1024 + toff0), p);                         // O^T[d = 4g+e][q = c]: V^T read transposed out of the row-major tile
      mma16(o1, rdtr(vs + kt * 1024 + toff1), p);
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.f / sum;
    o0 *= inv; o1 *= inv;
    if (q_ok) {
      bf16_t *o = out + ((int64_t)b * N + q) * C + h * D + 4 * g;
      st4(o, o0[0], o0[1], o0[2], o0[3]);
      st4(o + 16, o1[0], o1[1], o1[2], o1[3]);
      if (g == 0) lse[((int64_t)b * heads + h) * N + q] = m + log2f(sum);
    }
    if (u + 1 < n_units) stash(buf ^ 1);                                  // (free since the barrier above)
  }
}

template <bool MASK>
__global__ __launch_bounds__(THREADS) void wattn7_bwd(const bf16_t *__restrict__ qkv, const float *__restrict__ table,
                                                      const uint8_t *__restrict__ region, const uint8_t *__restrict__ flags,
                                                      const bf16_t *__restrict__ out, const bf16_t *__restrict__ dout,
                                                      const float *__restrict__ lse, bf16_t *__restrict__ dqkv,
                                                      float *__restrict__ dtable, int B_, int nW, int heads, float scale,
                                                      float c1, int chunk)
{
  __shared__ __attribute__((aligned(16))) unsigned char tiles[2 * 4 * TILE_B];  // [buffer][Q, K, V, dO]; after the last window: the [64][64] fp32 sum of dS
  __shared__ __attribute__((aligned(16))) float lse_all[2 * NP], delta_all[2 * NP];
  __shared__ __attribute__((aligned(16))) unsigned char reg_all[2 * NP];
  __shared__ float tbl[TBL];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 15, g = lane >> 4, h = blockIdx.y;
  const int C = heads * D;
  const int64_t ld = 3 * C;
  const int lrow = tid >> 2, lch = (tid & 3) ^ swz(lrow);
  const bool lrow_ok = lrow < N;
  const int b0 = blockIdx.x * chunk, n_units = min(chunk, B_ - b0);
  uint4 qn = {0u, 0u, 0u, 0u}, kn = qn, vn = qn, dn = qn, on = qn;        // (never loaded for a padded row: they stay 0)
  float ln = 0.f;
  unsigned rn = 0;
  auto fetch = [&](int b) {
    if (lrow_ok) {
      const bf16_t *base = qkv + ((int64_t)b * N + lrow) * ld + h * D + lch * 8;
      const int64_t go = ((int64_t)b * N + lrow) * C + h * D + lch * 8;
      qn = *reinterpret_cast<const uint4 *>(base);
      kn = *reinterpret_cast<const uint4 *>(base + C);
      vn = *reinterpret_cast<const uint4 *>(base + 2 * C);
      dn = *reinterpret_cast<const uint4 *>(dout + go);
      on = *reinterpret_cast<const uint4 *>(out + go);
    }
    if (tid < N) {
      ln = lse[((int64_t)b * heads + h) * N + tid];
      if (MASK) rn = region[(int64_t)(b % nW) * N + tid];
    }
  };
  auto stash = [&](int buf) {
    unsigned char *t = tiles + buf * 4 * TILE_B + tid * 16;
    if (lrow_ok) {
      *reinterpret_cast<uint4 *>(t) = qn;
      *reinterpret_cast<uint4 *>(t + TILE_B) = kn;
      *reinterpret_cast<uint4 *>(t + 2 * TILE_B) = vn;
      *reinterpret_cast<uint4 *>(t + 3 * TILE_B) = dn;
    }
    float acc = dot8(dn, on);                                             // delta = rowsum(dO * O): 4 threads per row (0 for a padded row)
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    if ((tid & 3) == 0) delta_all[buf * NP + lrow] = acc;
    if (tid < NP) {
      lse_all[buf * NP + tid] = tid < N ? ln : 0.f;
      if (MASK) reg_all[buf * NP + tid] = tid < N ? (unsigned char)rn : (unsigned char)0;
    }
  };
  fetch(b0);
  if (!lrow_ok) {                                                         // the padded rows of all eight tiles: zero, once
#pragma unroll
    for (int t = 0; t < 8; ++t) *reinterpret_cast<uint4 *>(tiles + t * TILE_B + tid * 16) = uint4{0u, 0u, 0u, 0u};
  }
  unsigned long long mbits = 0;
  if (MASK) mbits = __ballot(lane < n_units && flags[(b0 + (lane < n_units ? lane : 0)) % nW] != 0);
  for (int i = tid; i < TBL; i += THREADS) tbl[i] = table[i * heads + h] * LOG2E;
  stash(0);

  // table gradient: a lane meets the same 16 (query, key) pairs in every window, so it sums dS over the `chunk` windows in registers;
  // the pairs -> table-entry reduction happens once per workgroup (below)
  f32x4 dacc[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) dacc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int off0 = piece_at(c, g), off1 = piece_at(c, 4 + g), toff0 = piece_at(4 * g + (c >> 2), c & 3), toff1 = piece_at(4 * g + (c >> 2), 4 + (c & 3));
  const int tok = 16 * wv + c;                                            // this lane's key in phase 1, its query in phase 2
  const bool tok_ok = tok < N;
  const int at = rel_a(tok);

  for (int u = 0; u < n_units; ++u) {
    const int b = b0 + u, buf = u & 1;
    const unsigned char *qs = tiles + buf * 4 * TILE_B, *ks = qs + TILE_B, *vs = qs + 2 * TILE_B, *dos = qs + 3 * TILE_B;
    const float *lse_s = lse_all + buf * NP, *delta_s = delta_all + buf * NP;
    const unsigned char *r = reg_all + buf * NP;
    bf16_t *dbase = dqkv + (int64_t)b * N * ld + h * D;
    __syncthreads();                                                      // window u is in LDS; window u - 1 is done with
    if (u + 1 < n_units) fetch(b + 1);
    const bool masked = MASK && ((mbits >> u) & 1);
    const unsigned rt = masked ? r[tok] : 0u;
    {                                                                     // ---- phase 1: this wave's 16 KEYS -> dK, dV
      const bf16x4 k0 = rd8(ks + wv * 1024 + off0), k1 = rd8(ks + wv * 1024 + off1);
      const bf16x4 v0 = rd8(vs + wv * 1024 + off0), v1 = rd8(vs + wv * 1024 + off1);
      f32x4 dk0 = {0.f, 0.f, 0.f, 0.f}, dk1 = dk0, dv0 = dk0, dv1 = dk0;
#pragma unroll
      for (int qt = 0; qt < NT; ++qt) {
        const bf16x4 qa0 = rd8(qs + qt * 1024 + off0), qa1 = rd8(qs + qt * 1024 + off1);
        const bf16x4 da0 = rd8(dos + qt * 1024 + off0), da1 = rd8(dos + qt * 1024 + off1);
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = s;
        mma16(s, qa0, k0);                                                // S[q = 4g+e][key = c]
        mma16(s, qa1, k1);
        mma16(dp, da0, v0);
        mma16(dp, da1, v1);
        const bf16x4 dot0 = rdtr(dos + qt * 1024 + toff0), dot1 = rdtr(dos + qt * 1024 + toff1);      // dO^T, Q^T: rows 4 g .. 4 g + 3 of column c
        const bf16x4 qt0 = rdtr(qs + qt * 1024 + toff0), qt1 = rdtr(qs + qt * 1024 + toff1);
        const f32x4 L = *reinterpret_cast<const f32x4 *>(lse_s + 16 * qt + 4 * g), Dl = *reinterpret_cast<const f32x4 *>(delta_s + 16 * qt + 4 * g);
        unsigned rq = 0;
        if (masked) rq = *reinterpret_cast<const unsigned *>(r + 16 * qt + 4 * g);
        float p[4], ds[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int qq = 16 * qt + 4 * g + e;
          float t = fmaf(s[e], c1, tbl[rel_a(qq) - at + 84]);
          if (masked && ((rq >> (8 * e)) & 255u) != rt) t += MASKED;
          p[e] = qq < N ? __builtin_amdgcn_exp2f(t - L[e]) : 0.f;         // a padded query gives dK, dV nothing
          ds[e] = p[e] * (dp[e] - Dl[e]) * scale;
        }
        const bf16x4 pb = pack4(p[0], p[1], p[2], p[3]), dsb = pack4(ds[0], ds[1], ds[2], ds[3]);
        mma16(dv0, dot0, pb);                                             // dV^T[d = 4g+e][key = c]
        mma16(dv1, dot1, pb);
        mma16(dk0, qt0, dsb);
        mma16(dk1, qt1, dsb);
      }
      if (tok_ok) {
        bf16_t *dkp = dbase + C + tok * ld + 4 * g, *dvp = dbase + 2 * C + tok * ld + 4 * g;
        st4(dkp, dk0[0], dk0[1], dk0[2], dk0[3]);
        st4(dkp + 16, dk1[0], dk1[1], dk1[2], dk1[3]);
        st4(dvp, dv0[0], dv0[1], dv0[2], dv0[3]);
        st4(dvp + 16, dv1[0], dv1[1], dv1[2], dv1[3]);
      }
    }
    {                                                                     // ---- phase 2: this wave's 16 QUERIES -> dQ, dtable
      const bf16x4 q0 = rd8(qs + wv * 1024 + off0), q1 = rd8(qs + wv * 1024 + off1);
      const bf16x4 d0 = rd8(dos + wv * 1024 + off0), d1 = rd8(dos + wv * 1024 + off1);
      const float L = lse_s[tok], Dl = delta_s[tok];
      f32x4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        const bf16x4 ka0 = rd8(ks + kt * 1024 + off0), ka1 = rd8(ks + kt * 1024 + off1);
        const bf16x4 va0 = rd8(vs + kt * 1024 + off0), va1 = rd8(vs + kt * 1024 + off1);
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = s;
        mma16(s, ka0, q0);                                                // S^T[key = 4g+e][q = c]
        mma16(s, ka1, q1);
        mma16(dp, va0, d0);
        mma16(dp, va1, d1);
        const bf16x4 kt0 = rdtr(ks + kt * 1024 + toff0), kt1 = rdtr(ks + kt * 1024 + toff1);          // K^T: rows 4 g .. 4 g + 3 of column c
        unsigned rk = 0;
        if (masked) rk = *reinterpret_cast<const unsigned *>(r + 16 * kt + 4 * g);
        float ds[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = 16 * kt + 4 * g + e;
          float t = fmaf(s[e], c1, tbl[at - rel_a(key) + 84]);
          if (masked && ((rk >> (8 * e)) & 255u) != rt) t += MASKED;
          const float p = (key < N && tok_ok) ? __builtin_amdgcn_exp2f(t - L) : 0.f;   // padded keys weigh 0; a padded query gives dtable nothing
          ds[e] = p * (dp[e] - Dl);
        }
        const bf16x4 dsb = pack4(ds[0] * scale, ds[1] * scale, ds[2] * scale, ds[3] * scale);
        mma16(dq0, kt0, dsb);                                             // dQ^T[d = 4g+e][q = c]
        mma16(dq1, kt1, dsb);
        dacc[kt][0] += ds[0]; dacc[kt][1] += ds[1]; dacc[kt][2] += ds[2]; dacc[kt][3] += ds[3];
      }
      if (tok_ok) {
        bf16_t *dqp = dbase + tok * ld + 4 * g;
        st4(dqp, dq0[0], dq0[1], dq0[2], dq0[3]);
        st4(dqp + 16, dq1[0], dq1[1], dq1[2], dq1[3]);
      }
    }
    if (u + 1 < n_units) stash(buf ^ 1);                                  // (free since the barrier above)
  }
  // sum of dS over this workgroup's windows, [64 queries][64 keys] fp32, goes through the (now dead) tile space; thread i < 169 owns
  // table entry i = (dr + 6) * 13 + (dc + 6) and adds up the pairs (rq, cq) -> (rq - dr, cq - dc) it is made of: every real element
  // is read exactly once, a padded row or column never
  float *red = reinterpret_cast<float *>(tiles);
  __syncthreads();
  {
    float *row = red + tok * NP + 4 * g;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) *reinterpret_cast<f32x4 *>(row + 16 * kt) = dacc[kt];
  }
  __syncthreads();
  if (tid < TBL) {
    const int dr = tid / 13 - 6, dc = tid % 13 - 6;
    float tsum = 0.f;
#pragma unroll
    for (int rq = 0; rq < 7; ++rq) {
      const int rk = rq - dr;
      const bool row_ok = rk >= 0 && rk < 7;
#pragma unroll
      for (int cq = 0; cq < 7; ++cq) {                                    // fixed trip counts: the 49 loads pipeline
        const int ck = cq - dc;
        const bool ok = row_ok && ck >= 0 && ck < 7;
        const float v = red[ok ? (rq * 7 + cq) * NP + rk * 7 + ck : 0];
        tsum += ok ? v : 0.f;
      }
    }
    atomicAdd(dtable + tid * heads + h, tsum);
  }
}

int check(const void *qkv, const float *table, const uint8_t *region, const uint8_t *flags, int B_, int nW, int heads, const char *who)
{
  if (B_ < 0 || nW <= 0 || heads <= 0 || (B_ % nW) != 0)
    return pd_set_error(PD_ERR_INVALID_ARG, "%s: bad sizes B_=%d nW=%d heads=%d (B_ must be a multiple of nW)", who, B_, nW, heads);
  if (B_ == 0) return PD_OK;
  if (!qkv || !table) return pd_set_error(PD_ERR_INVALID_ARG, "%s: null input", who);
  if ((region == nullptr) != (flags == nullptr)) return pd_set_error(PD_ERR_INVALID_ARG, "%s: region and win_flags go together", who);
  if (((uintptr_t)qkv & 15) != 0) return pd_set_error(PD_ERR_INVALID_ARG, "%s: qkv must be 16-byte aligned", who);
  return PD_OK;
}

// windows one workgroup walks (<= 16), chosen as at window 12 to minimise (rounds of workgroups over the 256 CUs) x (windows + the
// per-workgroup fixed cost in window units: table staging and padded-row fill, and in the backward the table-gradient reduction and
// its 169 atomics)
int chunk_of(int B_, int heads, float fixed_cost, int wgs_per_cu)
{
  int best = 1;
  float best_cost = 1e30f;
  for (int chunk = 1; chunk <= MAX_CHUNK; ++chunk) {
    const int64_t wgs = (int64_t)heads * ((B_ + chunk - 1) / chunk);
    const int64_t rounds = (wgs + 256 * wgs_per_cu - 1) / (256 * wgs_per_cu);
    const float cost = rounds * (chunk + fixed_cost);
    if (cost < best_cost) { best_cost = cost; best = chunk; }
  }
  return best;
}
}  // namespace

extern "C" int pd_window_attn_fwd_w7(const void *qkv, const float *table, const uint8_t *region, const uint8_t *win_flags,
                                     void *out, float *lse, int B_, int nW, int heads, float scale, void *stream_)
{
  int rc = check(qkv, table, region, win_flags, B_, nW, heads, "pd_window_attn_fwd_w7");
  if (rc || B_ == 0) return rc;
  if (!out || !lse) return pd_set_error(PD_ERR_INVALID_ARG, "pd_window_attn_fwd_w7: null output");
  if (((uintptr_t)out & 7) != 0) return pd_set_error(PD_ERR_INVALID_ARG, "pd_window_attn_fwd_w7: out must be 8-byte aligned");
  const int chunk = g_pd_dbg_wattn_chunk ? g_pd_dbg_wattn_chunk : chunk_of(B_, heads, 0.5f, 4);
  const dim3 grid((B_ + chunk - 1) / chunk, heads);
  hipStream_t s = (hipStream_t)stream_;
  if (region) hipLaunchKernelGGL(wattn7_fwd<true>, grid, dim3(THREADS), 0, s, (const bf16_t *)qkv, table, region, win_flags, (bf16_t *)out, lse, B_, nW, heads, scale * LOG2E, chunk);
  else hipLaunchKernelGGL(wattn7_fwd<false>, grid, dim3(THREADS), 0, s, (const bf16_t *)qkv, table, region, win_flags, (bf16_t *)out, lse, B_, nW, heads, scale * LOG2E, chunk);
  return pd_check_launch("pd_window_attn_fwd_w7");
}

extern "C" int pd_window_attn_bwd_w7(const void *qkv, const float *table, const uint8_t *region, const uint8_t *win_flags,
                                     const void *out, const void *d_out, const float *lse, void *dqkv, float *dtable, int B_,
                                     int nW, int heads, float scale, void *stream_)
{
  int rc = check(qkv, table, region, win_flags, B_, nW, heads, "pd_window_attn_bwd_w7");
  if (rc || B_ == 0) return rc;
  if (!out || !d_out || !lse || !dqkv || !dtable) return pd_set_error(PD_ERR_INVALID_ARG, "pd_window_attn_bwd_w7: null pointer");
  if ((((uintptr_t)out | (uintptr_t)d_out | (uintptr_t)dqkv) & 15) != 0)
    return pd_set_error(PD_ERR_INVALID_ARG, "pd_window_attn_bwd_w7: out / d_out / dqkv must be 16-byte aligned");
  const int chunk = g_pd_dbg_wattn_chunk ? g_pd_dbg_wattn_chunk : chunk_of(B_, heads, 1.5f, 3);
  const dim3 grid((B_ + chunk - 1) / chunk, heads);
  hipStream_t s = (hipStream_t)stream_;
  if (region) hipLaunchKernelGGL(wattn7_bwd<true>, grid, dim3(THREADS), 0, s, (const bf16_t *)qkv, table, region, win_flags, (const bf16_t *)out, (const bf16_t *)d_out, lse, (bf16_t *)dqkv, dtable, B_, nW, heads, scale, scale * LOG2E, chunk);
  else hipLaunchKernelGGL(wattn7_bwd<false>, grid, dim3(THREADS), 0, s, (const bf16_t *)qkv, table, region, win_flags, (const bf16_t *)out, (const bf16_t *)d_out, lse, (bf16_t *)dqkv, dtable, B_, nW, heads, scale, scale * LOG2E, chunk);
  return pd_check_launch("pd_window_attn_bwd_w7");
}
