// Panoptic-parts uid decoder (include/pd_pparts.h): one streaming elementwise pass.  A thread takes four consecutive uids
// with one 16-byte load and stores each requested output with one 16-byte store (the uint8 labels with one 4-byte store); the up to
// three uids past the last whole group go to the first threads, one each.  Pointers that are not aligned that far take the same kernel
// with one uid per thread.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_msda.h"
#include "pd_pparts.h"

namespace {
struct Decoded {
  int sid, iid, pid;
  bool bad;
};

__device__ __forceinline__ Decoded decode_uid(int uid)
{
  Decoded d = {-1, -1, -1, (unsigned)uid > (unsigned)PD_PP_MAX_UID};          // negative uids wrap above the maximum
  if (d.bad) return d;
  if (uid < 100) {
    d.sid = uid;
  } else if (uid < 100000) {
    d.sid = uid / 1000;
    d.iid = uid % 1000;
  } else {
    d.sid = uid / 100000;
    d.iid = (uid / 100) % 1000;
    d.pid = uid % 100;
  }
  return d;
}

__device__ __forceinline__ void decode_one(const int32_t *uids, int64_t i, int32_t *sids, int32_t *iids, int32_t *pids, uint8_t *part_label,
                                           int32_t *invalid_flag)
{
  const Decoded d = decode_uid(uids[i]);
  if (sids) sids[i] = d.sid;
  if (iids) iids[i] = d.iid;
  if (pids) pids[i] = d.pid;
  if (part_label) part_label[i] = (uint8_t)(d.pid > 0 ? d.pid : 0);
  if (d.bad) *invalid_flag = 1;
}

template <bool VEC>
__global__ __launch_bounds__(256) void pp_decode(const int32_t *__restrict__ uids, int64_t numel, int32_t *__restrict__ sids,
                                                 int32_t *__restrict__ iids, int32_t *__restrict__ pids, uint8_t *__restrict__ part_label,
                                                 int32_t *__restrict__ invalid_flag)
{
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (!VEC) {
    if (t < numel) decode_one(uids, t, sids, iids, pids, part_label, invalid_flag);
    return;
  }
  const int64_t groups = numel / 4;
  if (t < groups) {
    const int4 u = reinterpret_cast<const int4 *>(uids)[t];
    const Decoded a = decode_uid(u.x), b = decode_uid(u.y), c = decode_uid(u.z), d = decode_uid(u.w);
    if (sids) reinterpret_cast<int4 *>(sids)[t] = make_int4(a.sid, b.sid, c.sid, d.sid);
    if (iids) reinterpret_cast<int4 *>(iids)[t] = make_int4(a.iid, b.iid, c.iid, d.iid);
    if (pids) reinterpret_cast<int4 *>(pids)[t] = make_int4(a.pid, b.pid, c.pid, d.pid);
    if (part_label)
      reinterpret_cast<uchar4 *>(part_label)[t] = make_uchar4((uint8_t)max(a.pid, 0), (uint8_t)max(b.pid, 0), (uint8_t)max(c.pid, 0),
                                                              (uint8_t)max(d.pid, 0));
    if (a.bad || b.bad || c.bad || d.bad) *invalid_flag = 1;
  }
  if (t < numel - 4 * groups) decode_one(uids, 4 * groups + t, sids, iids, pids, part_label, invalid_flag);
}

bool aligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }      // a null pointer is aligned
}  // namespace

extern "C" int pd_pp_decode_uids(const int32_t *uids, int64_t numel, int32_t *sids, int32_t *iids, int32_t *pids, uint8_t *part_label,
                                 int32_t *invalid_flag, void *stream_)
{
  if (numel < 0 || numel > ((int64_t)1 << 40)) return pd_set_error(PD_ERR_INVALID_ARG, "pd_pp_decode_uids: bad numel=%lld", (long long)numel);
  if (numel == 0) return PD_OK;
  if (!uids || !invalid_flag) return pd_set_error(PD_ERR_INVALID_ARG, "pd_pp_decode_uids: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = aligned(uids, 16) && aligned(sids, 16) && aligned(iids, 16) && aligned(pids, 16) && aligned(part_label, 4);
  const int64_t threads = !vec ? numel : numel / 4 > numel % 4 ? numel / 4 : numel % 4;     // whole groups, or the few uids past them
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  if (vec)
    hipLaunchKernelGGL(pp_decode<true>, dim3(blocks), dim3(256), 0, stream, uids, numel, sids, iids, pids, part_label, invalid_flag);
  else
    hipLaunchKernelGGL(pp_decode<false>, dim3(blocks), dim3(256), 0, stream, uids, numel, sids, iids, pids, part_label, invalid_flag);
  return pd_check_launch("pd_pp_decode_uids");
}
