// Evaluation counters (C-ABI: include/pd_eval.h): bit planes of masks, pairwise intersections, label-map confusion tables and the
// greedy cover of the box-proposal recall — every count an exact integer, a batch of images one launch per kernel.
//
// Workgroup -> work item: every grouped kernel gets a device table of entries, each with the index of its first workgroup
// (wg_begin, ascending); a workgroup finds its entry by a scan of the (short) table (grouped_table.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_eval.h"
#include "grouped_table.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int k)
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k);
  return ((uint64_t)hi << 32) | lo;
}

// ------------------------------------------------------------------------------------------------------------------- bit planes
// A thread turns 16 pixels (one 16-byte load, or 16 guarded byte loads at the tail / for unaligned rows) into 16 bits; the four
// lanes 4k .. 4k + 3 hold the four 16-bit pieces of one 64-bit word and OR them together.
constexpr int kPackPieces = 4;                                    // pieces of 16 pixels per thread
constexpr int64_t kPackPiecesPerWg = (int64_t)kThreads * kPackPieces;

struct PackEntry {
  const uint8_t *masks;
  uint64_t *bits;
  int64_t *area;
  int64_t hw, words;
  int32_t chunks, aligned;
  int64_t wg_begin;
};

__device__ __forceinline__ uint32_t nz_bits4(uint32_t x)          // bit k = (byte k of x != 0), k < 4
{
  x |= x >> 4;
  x |= x >> 2;
  x |= x >> 1;
  x &= 0x01010101u;
  return (x * 0x10204080u) >> 28;
}

__global__ void __launch_bounds__(kThreads) eval_pack(const PackEntry *table, int count)
{
  const PackEntry *e = find_entry(table, count, blockIdx.x);
  const int64_t local = blockIdx.x - e->wg_begin;
  const int64_t i = local / e->chunks, chunk = local % e->chunks;
  const int64_t hw = e->hw, words = e->words, pieces = words * 4;
  const uint8_t *src = pd_as_global(e->masks) + i * hw;
  uint64_t *dst = pd_as_global(e->bits) + i * words;
  const bool aligned = e->aligned;
  const int tid = threadIdx.x;
  uint32_t cnt = 0;
  for (int k = 0; k < kPackPieces; ++k) {
    const int64_t q = chunk * kPackPiecesPerWg + (int64_t)k * kThreads + tid;
    const int64_t px0 = q * 16;
    uint32_t piece = 0;
    if (q < pieces) {
      if (aligned && px0 + 16 <= hw) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src + px0);
        piece = nz_bits4(v.x) | (nz_bits4(v.y) << 4) | (nz_bits4(v.z) << 8) | (nz_bits4(v.w) << 12);
      } else {
        for (int j = 0; j < 16; ++j)
          if (px0 + j < hw) piece |= (uint32_t)(src[px0 + j] != 0) << j;
      }
    }
    cnt += __popc(piece);
    uint64_t word = (uint64_t)piece << (16 * (tid & 3));
    word |= __shfl_xor(word, 1);
    word |= __shfl_xor(word, 2);
    if ((tid & 3) == 0 && q < pieces) dst[q >> 2] = word;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  __shared__ uint32_t red[kThreads / 64];
  if ((tid & 63) == 0) red[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    const uint32_t s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(reinterpret_cast<unsigned long long *>(pd_as_global(e->area) + i), (unsigned long long)s);
  }
}

// ------------------------------------------------------------------------------------------------------------------- intersections
// A workgroup owns a tile of kTP rows x kTG columns and a span of kThreads * kKW words; a thread walks words w = tid, tid + 256, ...
// (coalesced), loads each operand word of the tile once and keeps the kTP x kTG counters in registers.  The tile's counters are
// reduced across the workgroup and added to the int64 result with one atomic each.
constexpr int kTP = 4, kTG = 16, kKW = 8;
constexpr int64_t kWordsPerWg = (int64_t)kThreads * kKW;

struct PairsEntry {
  const uint64_t *a;
  const int64_t *rows;
  const uint64_t *b;
  int64_t *inter;
  int64_t words;
  int32_t p, g, row_tiles, col_tiles, chunks, pad;
  int64_t wg_begin;
};

__global__ void __launch_bounds__(kThreads) eval_intersect(const PairsEntry *table, int count)
{
  const PairsEntry *e = find_entry(table, count, blockIdx.x);
  const int64_t local = blockIdx.x - e->wg_begin;
  const int64_t chunk = local % e->chunks, tile = local / e->chunks;
  const int ct = (int)(tile % e->col_tiles), rt = (int)(tile / e->col_tiles);
  const int64_t words = e->words;
  const int p = e->p, g = e->g;
  const int tid = threadIdx.x;
  const uint64_t *a = pd_as_global(e->a), *b = pd_as_global(e->b);
  const int64_t *rows = e->rows ? pd_as_global(e->rows) : nullptr;
  const uint64_t *ap[kTP];
  const uint64_t *bp[kTG];
#pragma unroll
  for (int i = 0; i < kTP; ++i) {
    const int r = rt * kTP + i;
    ap[i] = r < p ? a + (rows ? rows[r] : (int64_t)r) * words : nullptr;
  }
#pragma unroll
  for (int j = 0; j < kTG; ++j) {
    const int c = ct * kTG + j;
    bp[j] = c < g ? b + (int64_t)c * words : nullptr;
  }
  uint32_t cnt[kTP][kTG];
#pragma unroll
  for (int i = 0; i < kTP; ++i)
#pragma unroll
    for (int j = 0; j < kTG; ++j) cnt[i][j] = 0;
  for (int k = 0; k < kKW; ++k) {
    const int64_t w = chunk * kWordsPerWg + (int64_t)k * kThreads + tid;
    if (w >= words) break;
    uint64_t av[kTP], bv[kTG];
#pragma unroll
    for (int i = 0; i < kTP; ++i) av[i] = ap[i] ? ap[i][w] : 0;
#pragma unroll
    for (int j = 0; j < kTG; ++j) bv[j] = bp[j] ? bp[j][w] : 0;
#pragma unroll
    for (int i = 0; i < kTP; ++i)
#pragma unroll
      for (int j = 0; j < kTG; ++j) cnt[i][j] += __popcll(av[i] & bv[j]);
  }
  __shared__ uint32_t red[kThreads / 64][kTP * kTG];
#pragma unroll
  for (int i = 0; i < kTP; ++i)
#pragma unroll
    for (int j = 0; j < kTG; ++j) {
      uint32_t s = cnt[i][j];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if ((tid & 63) == 0) red[tid >> 6][i * kTG + j] = s;
    }
  __syncthreads();
  if (tid < kTP * kTG) {
    const int r = rt * kTP + tid / kTG, c = ct * kTG + tid % kTG;
    const uint32_t s = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (r < p && c < g && s)
      atomicAdd(reinterpret_cast<unsigned long long *>(pd_as_global(e->inter) + (int64_t)r * g + c), (unsigned long long)s);
  }
}

// ------------------------------------------------------------------------------------------------------------------- confusion table
// One wave per 64-pixel word, one lane per pixel.  A label is found by walking the masks from the last to the first, 64 mask words per
// (gathered) load, and stops as soon as every pixel of the word is covered.  Pixels with equal (pred, gt) bins are counted together
// (one add per distinct bin of the word).
constexpr int kConfWordsPerWave = 16;
constexpr int64_t kConfWordsPerWg = (int64_t)(kThreads / 64) * kConfWordsPerWave;

struct ConfEntry {
  const uint64_t *pb;
  const int64_t *pc;
  const uint64_t *gb;
  const int64_t *gc;
  const int64_t *slot;
  int64_t hw, words;
  int32_t pn, gn, chunks, pad;
  int64_t wg_begin;
};

// class of the last of the m masks covering this lane's pixel, n when none; -1 when that class lies outside [0, n]
__device__ __forceinline__ int last_label(const uint64_t *bits, const int64_t *cls, int m, int64_t words, int64_t w, uint64_t valid,
                                          int lane, int n)
{
  int lab = n;
  uint64_t assigned = ~valid;
  for (int top = m - 1; top >= 0 && assigned != ~0ull; top -= 64) {
    const int mi = top - lane;
    uint64_t v = 0;
    int c = 0;
    if (mi >= 0) {
      v = bits[(int64_t)mi * words + w];
      const int64_t c64 = cls[mi];
      c = (c64 < 0 || c64 > n) ? -1 : (int)c64;
    }
    const int kmax = top + 1 < 64 ? top + 1 : 64;
    for (int k = 0; k < kmax; ++k) {
      const uint64_t wk = readlane64(v, k);
      const int ck = __builtin_amdgcn_readlane(c, k);
      if (((wk & ~assigned) >> lane) & 1) lab = ck;
      assigned |= wk;
      if (assigned == ~0ull) break;
    }
  }
  return lab;
}

template <bool kLds>
__global__ void __launch_bounds__(kThreads) eval_confusion(const ConfEntry *table, int count, int n, int64_t *conf, int num_slots)
{
  extern __shared__ uint32_t hist[];
  const ConfEntry *e = find_entry(table, count, blockIdx.x);
  const int64_t slot = *pd_as_global(e->slot);
  if (slot < 0 || slot >= num_slots) return;                     // uniform: the whole workgroup leaves
  const int64_t bins = (int64_t)(n + 1) * (n + 1);
  int64_t *out = conf + slot * bins;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (kLds) {
    for (int64_t bi = tid; bi < bins; bi += kThreads) hist[bi] = 0;
    __syncthreads();
  }
  const int64_t chunk = blockIdx.x - e->wg_begin;
  const int64_t hw = e->hw, words = e->words;
  const uint64_t *pb = pd_as_global(e->pb), *gb = pd_as_global(e->gb);
  const int64_t *pc = pd_as_global(e->pc), *gc = pd_as_global(e->gc);
  for (int k = 0; k < kConfWordsPerWave; ++k) {
    const int64_t w = chunk * kConfWordsPerWg + (int64_t)wave * kConfWordsPerWave + k;
    if (w >= words) break;
    const int64_t left = hw - w * 64;
    const uint64_t valid = left >= 64 ? ~0ull : ((1ull << left) - 1);
    const int pl = last_label(pb, pc, e->pn, words, w, valid, lane, n);
    const int gl = last_label(gb, gc, e->gn, words, w, valid, lane, n);
    const bool ok = ((valid >> lane) & 1) && pl >= 0 && gl >= 0;
    const int bin = pl * (n + 1) + gl;
    uint64_t act = __ballot(ok);
    while (act) {
      const int leader = __ffsll((unsigned long long)act) - 1;
      const int b = __builtin_amdgcn_readlane(bin, leader);
      const uint64_t m = __ballot(bin == b) & act;
      if (lane == leader) {
        if (kLds) atomicAdd(&hist[b], (uint32_t)__popcll(m));
        else atomicAdd(reinterpret_cast<unsigned long long *>(out + b), (unsigned long long)__popcll(m));
      }
      act &= ~m;
    }
  }
  if (kLds) {
    __syncthreads();
    for (int64_t bi = tid; bi < bins; bi += kThreads)
      if (hist[bi]) atomicAdd(reinterpret_cast<unsigned long long *>(out + bi), (unsigned long long)hist[bi]);
  }
}

// ------------------------------------------------------------------------------------------------------------------- greedy cover
// One workgroup of PD_EVAL_LIMITS waves per image: the intersections of the kept columns go to LDS once, then wave l runs the greedy
// rounds of limit l with one lane per column.  A lane keeps its column's maximum over the rows still in play (and the first row
// reaching it); a round takes the largest (first column on ties), retires its row and column, and only the columns whose maximum sat
// in the retired row look at their rows again.  Retired rows and columns of the reference hold -1, below every IoU, so the maxima over
// the remaining rows / columns pick the same elements.
constexpr int kRecallThreads = PD_EVAL_LIMITS * 64;

struct RecallEntry {
  const int64_t *inter;
  const int64_t *rows;
  const int64_t *area_p, *area_g;
  int32_t p, g;
  int64_t wg_begin;
};

__device__ __forceinline__ double iou_of(uint32_t inter, int64_t ap, int64_t ag)
{
  const int64_t u = ap + ag - (int64_t)inter;
  return u > 0 ? (double)inter / (double)u : 0.0;
}

__global__ void __launch_bounds__(kRecallThreads) eval_recall(const RecallEntry *table, const float *thresholds, int64_t *hits,
                                                              int64_t *num_pos)
{
  __shared__ uint32_t inter_s[PD_EVAL_MAX_ROWS * PD_EVAL_MAX_GT];
  __shared__ int64_t ap_s[PD_EVAL_MAX_ROWS], ag_s[PD_EVAL_MAX_GT];
  __shared__ int colmap[PD_EVAL_MAX_GT];
  __shared__ int gf_s;
  const RecallEntry *e = pd_as_global(table + blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = e->p, g = e->g;
  if (wave == 0) {
    int64_t a = 0;
    if (lane < g) a = pd_as_global(e->area_g)[lane];
    const bool keep = lane < g && a > 0 && (double)a <= 1e10;
    const uint64_t bal = __ballot(keep);
    if (keep) {
      const int pos = __popcll(bal & ((1ull << lane) - 1));
      colmap[pos] = lane;
      ag_s[pos] = a;
    }
    if (lane == 0) gf_s = __popcll(bal);
  }
  __syncthreads();
  const int gf = gf_s;
  const int64_t *inter = pd_as_global(e->inter);
  const int64_t *rows = e->rows ? pd_as_global(e->rows) : nullptr;
  for (int idx = tid; idx < p * gf; idx += kRecallThreads) {
    const int r = idx / gf, c = idx - r * gf;
    inter_s[idx] = (uint32_t)inter[(int64_t)r * g + colmap[c]];
  }
  for (int r = tid; r < p; r += kRecallThreads) ap_s[r] = pd_as_global(e->area_p)[rows ? rows[r] : r];
  __syncthreads();

  const int limits[PD_EVAL_LIMITS] = {1, 10, 50, 100, 200};
  const int pr = p < limits[wave] ? p : limits[wave];
  const int rounds = pr < gf ? pr : gf;
  float thr[PD_EVAL_THRESHOLDS];
#pragma unroll
  for (int t = 0; t < PD_EVAL_THRESHOLDS; ++t) thr[t] = thresholds[t];
  uint64_t used[(PD_EVAL_MAX_ROWS + 63) / 64] = {0, 0, 0, 0};
  const int c = lane;
  bool live = c < gf;
  double best = -1.0;
  int arg = 0;
  auto column_max = [&]() {
    best = -1.0;
    arg = 0;
    for (int r = 0; r < pr; ++r) {
      if ((used[r >> 6] >> (r & 63)) & 1) continue;
      const double v = iou_of(inter_s[r * gf + c], ap_s[r], ag_s[c]);
      if (v > best) {
        best = v;
        arg = r;
      }
    }
  };
  if (live) column_max();
  int hitc[PD_EVAL_THRESHOLDS];
#pragma unroll
  for (int t = 0; t < PD_EVAL_THRESHOLDS; ++t) hitc[t] = 0;
  for (int round = 0; round < rounds; ++round) {
    double v = live ? best : -2.0;
    int ci = c;
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(v, off);
      const int oc = __shfl_xor(ci, off);
      if (ov > v || (ov == v && oc < ci)) {
        v = ov;
        ci = oc;
      }
    }
    const int rstar = __shfl(arg, ci);
    const float f = (float)v;
#pragma unroll
    for (int t = 0; t < PD_EVAL_THRESHOLDS; ++t) hitc[t] += f >= thr[t];
    used[rstar >> 6] |= 1ull << (rstar & 63);
    if (c == ci) live = false;
    if (live && arg == rstar) column_max();
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < PD_EVAL_THRESHOLDS; ++t)
      if (hitc[t]) atomicAdd(reinterpret_cast<unsigned long long *>(hits + wave * PD_EVAL_THRESHOLDS + t), (unsigned long long)hitc[t]);
    if (gf) atomicAdd(reinterpret_cast<unsigned long long *>(num_pos + wave), (unsigned long long)gf);
  }
}

}  // namespace

extern "C" int64_t pd_eval_table_bytes(int32_t count)
{
  size_t m = sizeof(PackEntry);
  if (sizeof(PairsEntry) > m) m = sizeof(PairsEntry);
  if (sizeof(ConfEntry) > m) m = sizeof(ConfEntry);
  if (sizeof(RecallEntry) > m) m = sizeof(RecallEntry);
  return (int64_t)(count > 0 ? count : 0) * (int64_t)m;
}

extern "C" int pd_eval_pack_grouped(const PdEvalMaskSet *list, int32_t count, void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<PackEntry>(
      "pd_eval_pack_grouped", list, count, true, table_host_pinned, table_device, st,
      [](const PdEvalMaskSet &d, int i, PackEntry &e, int64_t wg_begin) -> int64_t {
        if (d.n < 0 || d.hw <= 0 || d.hw >= (int64_t)1 << 32 || (d.n > 0 && (!d.masks || !d.bits || !d.area)))
          return pd_set_error(PD_ERR_INVALID_ARG, "pd_eval_pack_grouped: set %d: n >= 0, 0 < hw < 2^32 and non-null pointers required", i);
        const int64_t words = (d.hw + 63) / 64;
        const int64_t chunks = (words * 4 + kPackPiecesPerWg - 1) / kPackPiecesPerWg;
        const int aligned = (d.hw % 16 == 0) && (((uintptr_t)d.masks & 15) == 0);
        e = PackEntry{d.masks, d.bits, d.area, d.hw, words, (int32_t)chunks, aligned, wg_begin};
        return chunks * d.n;
      });
  if (wgs <= 0) return (int)wgs;
  hipLaunchKernelGGL(eval_pack, dim3((unsigned)wgs), dim3(kThreads), 0, st, (const PackEntry *)table_device, count);
  return pd_check_launch("pd_eval_pack_grouped");
}

extern "C" int pd_eval_intersect_grouped(const PdEvalPairs *list, int32_t count, void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<PairsEntry>(
      "pd_eval_intersect_grouped", list, count, true, table_host_pinned, table_device, st,
      [](const PdEvalPairs &d, int i, PairsEntry &e, int64_t wg_begin) -> int64_t {
        if (d.p < 1 || d.g < 1 || d.g > PD_EVAL_MAX_GT || d.words < 1 || !d.a || !d.b || !d.inter)
          return pd_set_error(PD_ERR_INVALID_ARG,
                              "pd_eval_intersect_grouped: pair %d: p >= 1, 1 <= g <= %d, words >= 1, non-null pointers required", i,
                              PD_EVAL_MAX_GT);
        const int32_t rt = (d.p + kTP - 1) / kTP, ct = (d.g + kTG - 1) / kTG;
        const int64_t chunks = (d.words + kWordsPerWg - 1) / kWordsPerWg;
        e = PairsEntry{d.a, d.rows, d.b, d.inter, d.words, d.p, d.g, rt, ct, (int32_t)chunks, 0, wg_begin};
        return (int64_t)rt * ct * chunks;
      });
  if (wgs <= 0) return (int)wgs;
  hipLaunchKernelGGL(eval_intersect, dim3((unsigned)wgs), dim3(kThreads), 0, st, (const PairsEntry *)table_device, count);
  return pd_check_launch("pd_eval_intersect_grouped");
}

extern "C" int pd_eval_confusion_grouped(const PdEvalConfusion *list, int32_t count, int32_t n, int64_t *conf, int32_t num_slots,
                                         void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<ConfEntry>(
      "pd_eval_confusion_grouped", list, count, conf != nullptr, table_host_pinned, table_device, st,
      [=](const PdEvalConfusion &d, int i, ConfEntry &e, int64_t wg_begin) -> int64_t {
        if (n < 1 || n > 46340 || num_slots < 1)                   // (the same for every i: answered at the first, before any descriptor)
          return pd_set_error(PD_ERR_INVALID_ARG, "pd_eval_confusion_grouped: n = %d, num_slots = %d", n, num_slots);
        if (d.pred_n < 0 || d.gt_n < 0 || d.hw <= 0 || !d.slot || (d.pred_n && (!d.pred_bits || !d.pred_cls)) ||
            (d.gt_n && (!d.gt_bits || !d.gt_cls)))
          return pd_set_error(PD_ERR_INVALID_ARG, "pd_eval_confusion_grouped: image %d: counts >= 0, hw > 0, non-null pointers required", i);
        const int64_t words = (d.hw + 63) / 64;
        const int64_t chunks = (words + kConfWordsPerWg - 1) / kConfWordsPerWg;
        e = ConfEntry{d.pred_bits, d.pred_cls, d.gt_bits, d.gt_cls, d.slot, d.hw, words, d.pred_n, d.gt_n, (int32_t)chunks, 0, wg_begin};
        return chunks;
      });
  if (wgs <= 0) return (int)wgs;
  const int64_t bins = (int64_t)(n + 1) * (n + 1);
  if (bins <= PD_EVAL_LDS_BINS)
    hipLaunchKernelGGL(eval_confusion<true>, dim3((unsigned)wgs), dim3(kThreads), (size_t)bins * sizeof(uint32_t), st,
                       (const ConfEntry *)table_device, count, n, conf, num_slots);
  else
    hipLaunchKernelGGL(eval_confusion<false>, dim3((unsigned)wgs), dim3(kThreads), 0, st, (const ConfEntry *)table_device, count, n, conf,
                       num_slots);
  return pd_check_launch("pd_eval_confusion_grouped");
}

extern "C" int pd_eval_recall_grouped(const PdEvalRecall *list, int32_t count, const float *thresholds, int64_t *hits, int64_t *num_pos,
                                      void *table_host_pinned, void *table_device, void *stream)
{
  hipStream_t st = (hipStream_t)stream;
  const int64_t wgs = stage_table<RecallEntry>(                    // one workgroup per image: wg_begin = i
      "pd_eval_recall_grouped", list, count, thresholds && hits && num_pos, table_host_pinned, table_device, st,
      [](const PdEvalRecall &d, int i, RecallEntry &e, int64_t wg_begin) -> int64_t {
        if (d.p < 1 || d.p > PD_EVAL_MAX_ROWS || d.g < 1 || d.g > PD_EVAL_MAX_GT || !d.inter || !d.area_p || !d.area_g)
          return pd_set_error(PD_ERR_INVALID_ARG, "pd_eval_recall_grouped: image %d: 1 <= p <= %d, 1 <= g <= %d, non-null pointers required", i,
                              PD_EVAL_MAX_ROWS, PD_EVAL_MAX_GT);
        e = RecallEntry{d.inter, d.rows, d.area_p, d.area_g, d.p, d.g, wg_begin};
        return 1;
      });
  if (wgs <= 0) return (int)wgs;
  hipLaunchKernelGGL(eval_recall, dim3((unsigned)wgs), dim3(kRecallThreads), 0, st, (const RecallEntry *)table_device, thresholds, hits,
                     num_pos);
  return pd_check_launch("pd_eval_recall_grouped");
}
