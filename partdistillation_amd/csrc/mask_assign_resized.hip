// Per-pixel mask assignment at a resized output and its histogram (C-ABI in include/pd_assign.h): the evaluation branch of the supervised
// model, and the assignment over (query, class) pairs of the class-aware branches.  Every kernel serves a batch of images in one launch through a device table of entries, each with the index of its first
// workgroup (wg_begin, ascending); a workgroup finds its entry by a scan of the (short) table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_assign.h"
#include "grouped_table.h"
#include "resize_taps.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kPx = 4;                       // pixels per lane of the assignment: 4 consecutive pixels of one output row
constexpr int kTileW = 64 * kPx;             // columns per workgroup
constexpr int kMixFloats = 1024;             // row-mixed logits a wavefront keeps in LDS: (k of one chunk) x (low-resolution columns under its 256 pixels)
constexpr int kMinChunk = 8;                 // fewest k per chunk for which the LDS row mix is used; a wider column span is read from memory
constexpr int kHistPx = 8;                   // consecutive pixels per thread and step of the histogram
constexpr int kHistSteps = 4;                // steps per workgroup: 8192 pixels
constexpr int kHistBins = 8192;              // int32 bins of a workgroup's LDS histogram

// ------------------------------------------------------------------------------------------------------------------- assignment
// One wavefront per output row segment of 256 pixels.  K runs up to 256, so the row mix of pd_scores_argmax_resized_u8 (the 4
// low-resolution rows of the output row combined once per (k, low column) into LDS) is walked in chunks of k that fit kMixFloats; the
// per-pixel state (best product, its k, the largest v) lives in registers across the chunks.  A segment whose column span leaves fewer
// than kMinChunk k per chunk (strong down-scaling) mixes per pixel from memory; the identity case evaluates pd_mask_assign's expression
// (src_index and bilinear2x2 of resize_taps.h, which csrc/grouping.hip uses too).
// Segments without an object pixel have v_k = 0 for every k: they write the first arg-max of the scores and obj = 0.
struct AssignEntry {
  const float *logits;
  const float *scores;
  const uint8_t *object;
  const int32_t *cls_of_query;
  int16_t *arg;
  uint8_t *obj;
  int32_t *positive;
  int16_t *cls;
  int32_t K, h, w, Hi, Wi, H, W, tiles_x, identity, pad;
  float sh1, sw1, sh2, sw2;
  int64_t wg_begin;
};

__global__ void __launch_bounds__(kThreads) mask_assign_resized(const AssignEntry *table, int count)
{
  __shared__ float mix_s[kWaves][kMixFloats];
  __shared__ int cnt[PD_ASSIGN_MAX_K];
  const AssignEntry *e = find_entry(table, count, blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = e->K, h = e->h, w = e->w, H = e->H, W = e->W;
  for (int i = tid; i < K; i += kThreads) cnt[i] = 0;
  const int64_t local = blockIdx.x - e->wg_begin;
  const int tx = (int)(local % e->tiles_x), ty = (int)(local / e->tiles_x);
  const int y = ty * kWaves + wave, xs = tx * kTileW, x0 = xs + lane * kPx;
  const bool row_ok = y < H;
  const float *logits = pd_as_global(e->logits);
  const float *scores = pd_as_global(e->scores);
  const uint8_t *object = pd_as_global(e->object);
  const int32_t *cls_of_query = pd_as_global(e->cls_of_query);
  int16_t *arg = pd_as_global(e->arg);
  uint8_t *obj = pd_as_global(e->obj);
  int32_t *positive = pd_as_global(e->positive);
  int16_t *cls = pd_as_global(e->cls);
  const int64_t o = (int64_t)y * W + x0;
  const int hw = h * w;

  bool in[kPx];
  float om[kPx];
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    in[j] = row_ok && x0 + j < W;
    om[j] = (in[j] && (!object || object[o + j])) ? 1.f : 0.f;
  }
  const bool any = __ballot(om[0] + om[1] + om[2] + om[3] != 0.f) != 0;        // wave-uniform: this segment has pixels that see the logits

  // the column span of the workgroup's 256 pixels is the same for its 4 rows: the chunk loop below is uniform over the workgroup
  const int xe = (xs + kTileW < W ? xs + kTileW : W) - 1;
  const int cmin = chain_of(xs, e->sw2, e->Wi, e->sw1, w).i[0];
  const int ncols = chain_of(xe, e->sw2, e->Wi, e->sw1, w).i[3] - cmin + 1;
  const bool identity = e->identity != 0;
  const bool use_lds = !identity && ncols * kMinChunk <= kMixFloats;
  const int kc = use_lds ? (kMixFloats / ncols < K ? kMixFloats / ncols : K) : K;

  float best[kPx], vmax[kPx];
  int besti[kPx];
#pragma unroll
  for (int j = 0; j < kPx; ++j) best[j] = -INFINITY, vmax[j] = -INFINITY, besti[j] = 0;

  // one k for the lane's 4 pixels: positive-pixel ballot, product with the score, running maxima
  auto consume = [&](int k, const float (&v)[kPx]) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < kPx; ++j) c += __popcll(__ballot(in[j] && v[j] > 0.f));
    if (lane == 0 && c) atomicAdd(&cnt[k], c);
    const float s = scores[k];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
      const float p = s * (1.f / (1.f + __expf(-v[j])));
      if (p > best[j]) {
        best[j] = p;
        besti[j] = k;
      }
      vmax[j] = fmaxf(vmax[j], v[j]);
    }
  };

  __syncthreads();                                                             // cnt is zero
  if (identity) {
    if (any) {
      int y0 = 0, yp = 0, c0[kPx], cp[kPx];
      float hy0 = 0.f, hy1 = 0.f, wx0[kPx], wx1[kPx];
      src_index(y, e->sh1, h, y0, yp, hy0, hy1);
#pragma unroll
      for (int j = 0; j < kPx; ++j) {
        c0[j] = cp[j] = 0, wx0[j] = wx1[j] = 0.f;
        if (in[j]) src_index(x0 + j, e->sw1, w, c0[j], cp[j], wx0[j], wx1[j]);
      }
      for (int k = 0; k < K; ++k) {
        const float *s = logits + k * hw;
        float v[kPx];
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
          v[j] = 0.f;
          if (in[j]) {
            const int a = y0 * w + c0[j], b = a + cp[j], c = (y0 + yp) * w + c0[j], d = c + cp[j];
            v[j] = bilinear2x2(s, a, b, c, d, hy0, hy1, wx0[j], wx1[j]) * om[j];
          }
        }
        consume(k, v);
      }
    }
  } else {
    Tap4 ry, cx[kPx];
    if (any) {
      ry = chain_of(y, e->sh2, e->Hi, e->sh1, h);
#pragma unroll
      for (int j = 0; j < kPx; ++j) cx[j] = chain_of(x0 + j < W ? x0 + j : W - 1, e->sw2, e->Wi, e->sw1, w);
    }
    auto rowmix = [&](int k, int c) {
      const float *s = logits + k * hw + c;
      return mix4(ry, [&](int i) { return s[i * w]; });
    };
    if (use_lds) {
      float *mix = mix_s[wave];
      for (int k0 = 0; k0 < K; k0 += kc) {
        const int kn = K - k0 < kc ? K - k0 : kc;
        if (any)
          for (int idx = lane; idx < kn * ncols; idx += 64) {
            const int k = idx / ncols, c = idx - k * ncols;
            mix[idx] = rowmix(k0 + k, cmin + c);
          }
        __syncthreads();
        if (any)
          for (int k = 0; k < kn; ++k) {
            const int b = k * ncols - cmin;
            float v[kPx];
#pragma unroll
            for (int j = 0; j < kPx; ++j)
              v[j] = mix4(cx[j], [=](int i) { return mix[b + i]; }) * om[j];
            consume(k0 + k, v);
          }
        __syncthreads();
      }
    } else if (any) {
      for (int k = 0; k < K; ++k) {
        float v[kPx];
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
          v[j] = 0.f;
          if (in[j])
            v[j] = mix4(cx[j], [&](int i) { return rowmix(k, i); }) * om[j];
        }
        consume(k, v);
      }
    }
  }
  if (!any) {                                                                  // v_k = 0 everywhere: sigmoid = 0.5, the first largest score wins
    float b = -INFINITY;
    int bi = 0;
    for (int k = 0; k < K; ++k) {
      const float p = scores[k] * 0.5f;
      if (p > b) b = p, bi = k;
    }
#pragma unroll
    for (int j = 0; j < kPx; ++j) besti[j] = bi;
  }

  if (in[0]) {
    uint8_t ob[kPx];
    int16_t cl[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
      ob[j] = vmax[j] > 0.f ? 1 : 0;
      cl[j] = -1;
    }
    if (cls_of_query && cls) {
#pragma unroll
      for (int j = 0; j < kPx; ++j)
        if (in[j] && ob[j]) cl[j] = (int16_t)cls_of_query[besti[j]];
    }
    int16_t *ap = arg + o;
    uint8_t *op = obj + o;
    const bool full = in[kPx - 1];
    store4_i16(ap, full && aligned8(ap), in, besti);
    store4_u8(op, full && aligned4(op), in, pack4_u8(ob));
    if (cls) {
      int16_t *cp = cls + o;
      if (full && aligned8(cp)) {                                              // (written out: store4_i16 here changes the kernel's instruction stream)
        uint2 v;
        v.x = (uint32_t)(uint16_t)cl[0] | ((uint32_t)(uint16_t)cl[1] << 16);
        v.y = (uint32_t)(uint16_t)cl[2] | ((uint32_t)(uint16_t)cl[3] << 16);
        *reinterpret_cast<uint2 *>(cp) = v;
      } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j)
          if (in[j]) cp[j] = cl[j];
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < K; k += kThreads)
    if (cnt[k]) atomicAdd(positive + k, cnt[k]);
}

// ------------------------------------------------------------------------------------------------------------------- assignment of pairs
// The same pass for K (query, class) pairs over Q shared logit maps (pd_pair_assign_resized).  At entry a workgroup threads the pairs
// of every query into an LDS list (head[q] -> pair -> next pair; LDS exchanges, so the order inside a list is arbitrary) and compacts the
// referenced queries, ascending, into qrec.  The chunk loop of mask_assign_resized then runs over qrec: row mix, the 4 x 4 taps, the
// positive-pixel count and the sigmoid happen once per referenced query, and the query's pairs only multiply by their score.  Pairs are
// visited grouped by query, so "first maximum in pair order" is an explicit rule: a product wins when it is larger, or equal with a
// smaller pair index.  Every arithmetic expression is the one of mask_assign_resized: the outputs are its outputs on logits[pair_query].
struct PairEntry {
  const float *logits;
  const int32_t *pair_query;
  const float *scores;
  const uint8_t *object;
  const int32_t *cls_of_pair;
  int16_t *arg;
  uint8_t *obj;
  int32_t *positive;
  int16_t *cls;
  int32_t K, Q, h, w, Hi, Wi, H, W, tiles_x, identity;
  float sh1, sw1, sh2, sw2;
  int64_t wg_begin;
};

struct PairNode {
  float score;
  int next;                                  // next pair of the same query, -1 at the end
};

// a referenced query with the first pair of its list: one 16-byte LDS read whose address depends on the loop counter alone, so a query
// with a single pair (most of them) costs no chain of dependent reads
struct QueryRec {
  float score;
  int k, next, q;
};

__global__ void __launch_bounds__(kThreads) pair_assign_resized(const PairEntry *table, int count)
{
  __shared__ float mix_s[kWaves][kMixFloats];
  __shared__ int head[PD_ASSIGN_MAX_Q];      // first pair of a query, -1: not referenced
  __shared__ PairNode node[PD_ASSIGN_MAX_K];
  __shared__ int cnt[PD_ASSIGN_MAX_K];       // positive pixels per referenced query (index into qrec)
  __shared__ QueryRec qrec[PD_ASSIGN_MAX_K]; // referenced queries, ascending
  __shared__ int nq_s;
  const PairEntry *e = find_entry(table, count, blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = e->K, Q = e->Q, h = e->h, w = e->w, H = e->H, W = e->W;
  const float *logits = pd_as_global(e->logits);
  const int32_t *pair_query = pd_as_global(e->pair_query);
  const float *scores = pd_as_global(e->scores);
  const uint8_t *object = pd_as_global(e->object);
  const int32_t *cls_of_pair = pd_as_global(e->cls_of_pair);
  int16_t *arg = pd_as_global(e->arg);
  uint8_t *obj = pd_as_global(e->obj);
  int32_t *positive = pd_as_global(e->positive);
  int16_t *cls = pd_as_global(e->cls);

  for (int i = tid; i < Q; i += kThreads) head[i] = -1;
  for (int i = tid; i < K; i += kThreads) cnt[i] = 0;
  __syncthreads();
  for (int k = tid; k < K; k += kThreads) {
    const int q = pair_query[k];
    PairNode n;
    n.score = scores[k];
    n.next = -2;                                                               // outside [0, Q): in no list, never wins
    if ((unsigned)q < (unsigned)Q) n.next = atomicExch(&head[q], k);
    node[k] = n;
  }
  __syncthreads();
  if (wave == 0) {                                                             // at most K queries are referenced
    int base = 0;
    for (int q0 = 0; q0 < Q; q0 += 64) {
      const int q = q0 + lane;
      const int k = q < Q ? head[q] : -1;
      const bool r = k >= 0;
      const unsigned long long b = __ballot(r);
      if (r) {
        const PairNode n = node[k];
        qrec[base + __popcll(b & ((1ull << lane) - 1ull))] = QueryRec{n.score, k, n.next, q};
      }
      base += __popcll(b);
    }
    if (lane == 0) nq_s = base;
  }
  __syncthreads();
  const int nq = nq_s;

  const int64_t local = blockIdx.x - e->wg_begin;
  const int tx = (int)(local % e->tiles_x), ty = (int)(local / e->tiles_x);
  const int y = ty * kWaves + wave, xs = tx * kTileW, x0 = xs + lane * kPx;
  const bool row_ok = y < H;
  const int64_t o = (int64_t)y * W + x0;
  const int hw = h * w;

  bool in[kPx];
  float om[kPx];
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    in[j] = row_ok && x0 + j < W;
    om[j] = (in[j] && (!object || object[o + j])) ? 1.f : 0.f;
  }
  const bool any = __ballot(om[0] + om[1] + om[2] + om[3] != 0.f) != 0;        // wave-uniform: this segment has pixels that see the logits

  const int xe = (xs + kTileW < W ? xs + kTileW : W) - 1;
  const int cmin = chain_of(xs, e->sw2, e->Wi, e->sw1, w).i[0];
  const int ncols = chain_of(xe, e->sw2, e->Wi, e->sw1, w).i[3] - cmin + 1;
  const bool identity = e->identity != 0;
  const bool use_lds = !identity && ncols * kMinChunk <= kMixFloats;           // the very condition of mask_assign_resized
  const int kc = use_lds ? (kMixFloats / ncols < nq ? kMixFloats / ncols : nq) : nq;

  float best[kPx], vmax[kPx];
  int besti[kPx];
#pragma unroll
  for (int j = 0; j < kPx; ++j) best[j] = -INFINITY, vmax[j] = -INFINITY, besti[j] = 0;

  // one referenced query (qrec[ci]) for the lane's 4 pixels: positive-pixel ballot and sigmoid once, then its pairs
  auto consume = [&](int ci, const float (&v)[kPx]) {
    const QueryRec r = qrec[ci];
    int c = 0;
#pragma unroll
    for (int j = 0; j < kPx; ++j) c += __popcll(__ballot(in[j] && v[j] > 0.f));
    if (lane == 0 && c) atomicAdd(&cnt[ci], c);
    float sig[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
      sig[j] = 1.f / (1.f + __expf(-v[j]));
      vmax[j] = fmaxf(vmax[j], v[j]);
    }
    float s = r.score;
    for (int k = r.k, next = r.next;;) {
      k = __builtin_amdgcn_readfirstlane(k);                                   // (uniform: ci is)
#pragma unroll
      for (int j = 0; j < kPx; ++j) {
        const float p = s * sig[j];
        if (p > best[j] || (p == best[j] && k < besti[j])) {
          best[j] = p;
          besti[j] = k;
        }
      }
      k = __builtin_amdgcn_readfirstlane(next);
      if (k < 0) break;
      const PairNode n = node[k];
      s = n.score, next = n.next;
    }
  };

  if (identity) {
    if (any) {
      int y0 = 0, yp = 0, c0[kPx], cp[kPx];
      float hy0 = 0.f, hy1 = 0.f, wx0[kPx], wx1[kPx];
      src_index(y, e->sh1, h, y0, yp, hy0, hy1);
#pragma unroll
      for (int j = 0; j < kPx; ++j) {
        c0[j] = cp[j] = 0, wx0[j] = wx1[j] = 0.f;
        if (in[j]) src_index(x0 + j, e->sw1, w, c0[j], cp[j], wx0[j], wx1[j]);
      }
      for (int ci = 0; ci < nq; ++ci) {
        const float *s = logits + qrec[ci].q * hw;
        float v[kPx];
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
          v[j] = 0.f;
          if (in[j]) {
            const int a = y0 * w + c0[j], b = a + cp[j], c = (y0 + yp) * w + c0[j], d = c + cp[j];
            v[j] = bilinear2x2(s, a, b, c, d, hy0, hy1, wx0[j], wx1[j]) * om[j];
          }
        }
        consume(ci, v);
      }
    }
  } else {
    Tap4 ry, cx[kPx];
    if (any) {
      ry = chain_of(y, e->sh2, e->Hi, e->sh1, h);
#pragma unroll
      for (int j = 0; j < kPx; ++j) cx[j] = chain_of(x0 + j < W ? x0 + j : W - 1, e->sw2, e->Wi, e->sw1, w);
    }
    auto rowmix = [&](int q, int c) {
      const float *s = logits + q * hw + c;
      return mix4(ry, [&](int i) { return s[i * w]; });
    };
    if (use_lds) {
      float *mix = mix_s[wave];
      for (int c0 = 0; c0 < nq; c0 += kc) {
        const int kn = nq - c0 < kc ? nq - c0 : kc;
        if (any)
          for (int idx = lane; idx < kn * ncols; idx += 64) {
            const int k = idx / ncols, c = idx - k * ncols;
            mix[idx] = rowmix(qrec[c0 + k].q, cmin + c);
          }
        __syncthreads();
        if (any)
          for (int k = 0; k < kn; ++k) {
            const int b = k * ncols - cmin;
            float v[kPx];
#pragma unroll
            for (int j = 0; j < kPx; ++j)
              v[j] = mix4(cx[j], [=](int i) { return mix[b + i]; }) * om[j];
            consume(c0 + k, v);
          }
        __syncthreads();
      }
    } else if (any) {
      for (int ci = 0; ci < nq; ++ci) {
        const int q = qrec[ci].q;
        float v[kPx];
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
          v[j] = 0.f;
          if (in[j])
            v[j] = mix4(cx[j], [&](int i) { return rowmix(q, i); }) * om[j];
        }
        consume(ci, v);
      }
    }
  }
  if (!any) {                                                                  // v = 0 everywhere: sigmoid = 0.5, the first largest score wins
    float b = -INFINITY;
    int bi = 0;
    for (int k = 0; k < K; ++k) {
      const float p = node[k].score * 0.5f;
      if (p > b && node[k].next != -2) b = p, bi = k;
    }
#pragma unroll
    for (int j = 0; j < kPx; ++j) besti[j] = bi;
  }

  if (in[0]) {
    uint8_t ob[kPx];
    int cl[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
      ob[j] = vmax[j] > 0.f ? 1 : 0;
      cl[j] = -1;
    }
    if (cls_of_pair && cls) {
#pragma unroll
      for (int j = 0; j < kPx; ++j)
        if (in[j] && ob[j]) cl[j] = cls_of_pair[besti[j]];
    }
    int16_t *ap = arg + o;
    uint8_t *op = obj + o;
    const bool full = in[kPx - 1];
    store4_i16(ap, full && aligned8(ap), in, besti);
    store4_u8(op, full && aligned4(op), in, pack4_u8(ob));
    if (cls) {
      int16_t *cp = cls + o;
      store4_i16(cp, full && aligned8(cp), in, cl);
    }
  }
  __syncthreads();
  for (int ci = tid; ci < nq; ci += kThreads) {                                // positive[k] is the count of its query
    const int c = cnt[ci];
    if (!c) continue;
    for (int k = qrec[ci].k; k >= 0; k = node[k].next) atomicAdd(positive + k, c);
  }
}

// ------------------------------------------------------------------------------------------------------------------- histogram
// A workgroup owns 8192 consecutive pixels; a thread reads 8 consecutive pixels per step (one 16-byte load of keys, 8-byte loads of the
// object map and of each ground-truth mask) and adds RUNS of equal keys to the LDS bins (assignment maps are piecewise constant, so one
// atomic per pixel would serialise on a few addresses).  Bins of a pass: won[n], area[n], inter[n][Gc], gt_area[Gc]; when n * (G + 2) + G
// exceeds kHistBins the ground-truth masks are walked in passes of Gc.  Non-zero bins reach memory by one 64-bit atomic each.
struct HistEntry {
  const int16_t *key;
  const uint8_t *obj;
  const uint8_t *gt;
  int64_t *won, *area, *inter, *gt_area;
  int32_t n, G;
  int64_t hw;
  int64_t wg_begin;
};

__device__ __forceinline__ uint64_t load_bytes8(const uint8_t *p, int cnt)
{
  if (cnt == kHistPx && ((uintptr_t)p & 7) == 0) return *reinterpret_cast<const uint64_t *>(p);
  uint64_t v = 0;
#pragma unroll
  for (int j = 0; j < kHistPx; ++j)
    if (j < cnt) v |= (uint64_t)p[j] << (8 * j);
  return v;
}

// 0x80 in every non-zero byte
__device__ __forceinline__ uint64_t nonzero_bytes(uint64_t m)
{
  const uint64_t lo = 0x7f7f7f7f7f7f7f7full;
  return (((m & lo) + lo) | m) & ~lo;
}

__device__ __forceinline__ void add64(int64_t *p, int v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }

__global__ void __launch_bounds__(kThreads) assign_histogram(const HistEntry *table, int count)
{
  __shared__ int bins[kHistBins];
  const HistEntry *e = find_entry(table, count, blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = e->n, G = e->G;
  const int64_t hw = e->hw;
  const int16_t *key = pd_as_global(e->key);
  const uint8_t *obj = pd_as_global(e->obj);
  const uint8_t *gt = pd_as_global(e->gt);
  int64_t *won = pd_as_global(e->won), *area = pd_as_global(e->area), *inter = pd_as_global(e->inter), *gt_area = pd_as_global(e->gt_area);
  const int64_t base = (blockIdx.x - e->wg_begin) * (int64_t)(kThreads * kHistPx * kHistSteps);
  int Gc = (kHistBins - 2 * n) / (n + 1);
  Gc = Gc < G ? Gc : G;
  for (int g0 = 0; g0 == 0 || g0 < G; g0 += Gc) {                             // (G == 0: one pass for won and area)
    const int gn = G - g0 < Gc ? G - g0 : Gc;
    const int total = 2 * n + n * gn + gn;
    for (int i = tid; i < total; i += kThreads) bins[i] = 0;
    __syncthreads();
    for (int step = 0; step < kHistSteps; ++step) {
      const int64_t p = base + ((int64_t)step * kThreads + tid) * kHistPx;
      const int64_t left = hw - p;
      const int c = left >= kHistPx ? kHistPx : (left > 0 ? (int)left : 0);
      int k[kHistPx];
      uint64_t ok = 0;                                                         // 0x80 in the bytes of pixels with a key in [0, n) and obj set
      if (c > 0) {
        const int16_t *kp = key + p;
        if (c == kHistPx && ((uintptr_t)kp & 15) == 0) {
          const uint4 v = *reinterpret_cast<const uint4 *>(kp);
          k[0] = (int16_t)(v.x & 0xffff), k[1] = (int16_t)(v.x >> 16), k[2] = (int16_t)(v.y & 0xffff), k[3] = (int16_t)(v.y >> 16);
          k[4] = (int16_t)(v.z & 0xffff), k[5] = (int16_t)(v.z >> 16), k[6] = (int16_t)(v.w & 0xffff), k[7] = (int16_t)(v.w >> 16);
        } else {
#pragma unroll
          for (int j = 0; j < kHistPx; ++j) k[j] = j < c ? (int)kp[j] : -1;
        }
        const uint64_t ob = nonzero_bytes(load_bytes8(obj + p, c));
#pragma unroll
        for (int j = 0; j < kHistPx; ++j) {
          if (k[j] < 0 || k[j] >= n) k[j] = -1;
          if (k[j] >= 0) ok |= ob & (0x80ull << (8 * j));
        }
        if (g0 == 0) {                                                         // won and area: runs of equal keys
          int cur = -1, cw = 0, ca = 0;
#pragma unroll
          for (int j = 0; j < kHistPx; ++j) {
            if (k[j] != cur) {
              if (cur >= 0) {
                atomicAdd(&bins[cur], cw);
                if (ca) atomicAdd(&bins[n + cur], ca);
              }
              cur = k[j], cw = 0, ca = 0;
            }
            cw += 1;
            ca += (int)((ok >> (8 * j + 7)) & 1);
          }
          if (cur >= 0) {
            atomicAdd(&bins[cur], cw);
            if (ca) atomicAdd(&bins[n + cur], ca);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < kHistPx; ++j) k[j] = -1;
      }
      for (int jj = 0; jj < gn; ++jj) {
        uint64_t m = 0;
        if (c > 0) m = nonzero_bytes(load_bytes8(gt + (int64_t)(g0 + jj) * hw + p, c));
        int ga = __popcll(m);
        for (int off = 32; off > 0; off >>= 1) ga += __shfl_xor(ga, off);
        if (lane == 0 && ga) atomicAdd(&bins[2 * n + n * gn + jj], ga);
        m &= ok;
        if (m) {
          int cur = -1, ci = 0;
#pragma unroll
          for (int j = 0; j < kHistPx; ++j) {
            const int t = (int)((m >> (8 * j + 7)) & 1);
            const int kk = t ? k[j] : -1;
            if (kk != cur) {
              if (cur >= 0) atomicAdd(&bins[2 * n + cur * gn + jj], ci);
              cur = kk, ci = 0;
            }
            ci += 1;
          }
          if (cur >= 0) atomicAdd(&bins[2 * n + cur * gn + jj], ci);
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < total; i += kThreads) {
      const int v = bins[i];
      if (!v) continue;
      if (i < n) add64(won + i, v);
      else if (i < 2 * n) add64(area + (i - n), v);
      else if (i < 2 * n + n * gn) {
        const int r = i - 2 * n, kk = r / gn, jj = r - kk * gn;
        add64(inter + (int64_t)kk * G + g0 + jj, v);
      } else add64(gt_area + g0 + (i - 2 * n - n * gn), v);
    }
    __syncthreads();
    if (Gc <= 0) break;
  }
}

}  // namespace

extern "C" int64_t pd_assign_table_bytes(int32_t count)
{
  size_t m = sizeof(AssignEntry) > sizeof(HistEntry) ? sizeof(AssignEntry) : sizeof(HistEntry);
  m = m > sizeof(PairEntry) ? m : sizeof(PairEntry);
  return (int64_t)(count > 0 ? count : 0) * (int64_t)m;
}

extern "C" int pd_mask_assign_resized(const PdAssignResized *list, int32_t count, void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<AssignEntry>(
      "pd_mask_assign_resized", list, count, true, table_host_pinned, table_device, st,
      [](const PdAssignResized &d, int i, AssignEntry &e, int64_t wg_begin) -> int64_t {
        if (d.K < 1 || d.K > PD_ASSIGN_MAX_K || d.h <= 0 || d.w <= 0 || d.Hp <= 0 || d.Wp <= 0 || d.Hi <= 0 || d.Wi <= 0 || d.Hi > d.Hp ||
            d.Wi > d.Wp || d.H <= 0 || d.W <= 0 || (int64_t)d.K * d.h * d.w >= INT32_MAX || !d.logits || !d.scores || !d.arg || !d.obj ||
            !d.positive)
          return pd_set_error(PD_ERR_INVALID_ARG,
                              "pd_mask_assign_resized: image %d: K=%d h=%d w=%d Hp=%d Wp=%d Hi=%d Wi=%d H=%d W=%d (1 <= K <= %d, Hi <= Hp, "
                              "Wi <= Wp, non-null logits / scores / arg / obj / positive required)",
                              i, d.K, d.h, d.w, d.Hp, d.Wp, d.Hi, d.Wi, d.H, d.W, PD_ASSIGN_MAX_K);
        const int32_t tiles_x = (d.W + kTileW - 1) / kTileW, tiles_y = (d.H + kWaves - 1) / kWaves;
        e = AssignEntry{d.logits, d.scores, d.object, d.cls_of_query, d.arg, d.obj, d.positive, d.cls, d.K, d.h, d.w, d.Hi, d.Wi, d.H, d.W,
                        tiles_x, (d.H == d.Hi && d.W == d.Wi) ? 1 : 0, 0,
                        (float)d.h / (float)d.Hp, (float)d.w / (float)d.Wp, (float)d.Hi / (float)d.H, (float)d.Wi / (float)d.W, wg_begin};
        return (int64_t)tiles_x * tiles_y;
      });
  if (wgs <= 0) return (int)wgs;
  hipLaunchKernelGGL(mask_assign_resized, dim3((unsigned)wgs), dim3(kThreads), 0, st, (const AssignEntry *)table_device, count);
  return pd_check_launch("pd_mask_assign_resized");
}

extern "C" int pd_pair_assign_resized(const PdAssignPairs *list, int32_t count, void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<PairEntry>(
      "pd_pair_assign_resized", list, count, true, table_host_pinned, table_device, st,
      [](const PdAssignPairs &d, int i, PairEntry &e, int64_t wg_begin) -> int64_t {
        if (d.K < 1 || d.K > PD_ASSIGN_MAX_K || d.Q < 1 || d.Q > PD_ASSIGN_MAX_Q || d.h <= 0 || d.w <= 0 || d.Hp <= 0 || d.Wp <= 0 ||
            d.Hi <= 0 || d.Wi <= 0 || d.Hi > d.Hp || d.Wi > d.Wp || d.H <= 0 || d.W <= 0 || (int64_t)d.Q * d.h * d.w >= INT32_MAX ||
            !d.logits || !d.pair_query || !d.scores || !d.arg || !d.obj || !d.positive)
          return pd_set_error(PD_ERR_INVALID_ARG,
                              "pd_pair_assign_resized: image %d: K=%d Q=%d h=%d w=%d Hp=%d Wp=%d Hi=%d Wi=%d H=%d W=%d (1 <= K <= %d, "
                              "1 <= Q <= %d, Hi <= Hp, Wi <= Wp, non-null logits / pair_query / scores / arg / obj / positive required)",
                              i, d.K, d.Q, d.h, d.w, d.Hp, d.Wp, d.Hi, d.Wi, d.H, d.W, PD_ASSIGN_MAX_K, PD_ASSIGN_MAX_Q);
        const int32_t tiles_x = (d.W + kTileW - 1) / kTileW, tiles_y = (d.H + kWaves - 1) / kWaves;
        e = PairEntry{d.logits, d.pair_query, d.scores, d.object, d.cls_of_pair, d.arg, d.obj, d.positive, d.cls, d.K, d.Q, d.h, d.w, d.Hi,
                      d.Wi, d.H, d.W, tiles_x, (d.H == d.Hi && d.W == d.Wi) ? 1 : 0,
                      (float)d.h / (float)d.Hp, (float)d.w / (float)d.Wp, (float)d.Hi / (float)d.H, (float)d.Wi / (float)d.W, wg_begin};
        return (int64_t)tiles_x * tiles_y;
      });
  if (wgs <= 0) return (int)wgs;
  hipLaunchKernelGGL(pair_assign_resized, dim3((unsigned)wgs), dim3(kThreads), 0, st, (const PairEntry *)table_device, count);
  return pd_check_launch("pd_pair_assign_resized");
}

extern "C" int pd_assign_histogram(const PdAssignHistogram *list, int32_t count, void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<HistEntry>(
      "pd_assign_histogram", list, count, true, table_host_pinned, table_device, st,
      [](const PdAssignHistogram &d, int i, HistEntry &e, int64_t wg_begin) -> int64_t {
        if (d.n < 1 || d.n > PD_ASSIGN_MAX_KEYS || d.G < 0 || d.G > PD_ASSIGN_MAX_GT || d.hw <= 0 || !d.key || !d.obj || !d.won || !d.area ||
            (d.G > 0 && (!d.gt || !d.inter || !d.gt_area)))
          return pd_set_error(PD_ERR_INVALID_ARG,
                              "pd_assign_histogram: image %d: n=%d G=%d hw=%lld (1 <= n <= %d, 0 <= G <= %d, hw > 0, non-null pointers required)",
                              i, d.n, d.G, (long long)d.hw, PD_ASSIGN_MAX_KEYS, PD_ASSIGN_MAX_GT);
        const int64_t per_wg = (int64_t)kThreads * kHistPx * kHistSteps;
        e = HistEntry{d.key, d.obj, d.gt, d.won, d.area, d.inter, d.gt_area, d.n, d.G, d.hw, wg_begin};
        return (d.hw + per_wg - 1) / per_wg;
      });
  if (wgs <= 0) return (int)wgs;
  hipLaunchKernelGGL(assign_histogram, dim3((unsigned)wgs), dim3(kThreads), 0, st, (const HistEntry *)table_device, count);
  return pd_check_launch("pd_assign_histogram");
}
