// Entry tables of the grouped evaluation launches (evaluation.hip, pixel_grouping.hip, mask_assign_resized.hip): a batch of images is
// one launch through a device table of entries, each with the index of its first workgroup (wg_begin, ascending).  The host fills the
// table in a pinned buffer and uploads it; a workgroup finds its entry by a scan of the (short) table.
#ifndef PD_GROUPED_TABLE_H
#define PD_GROUPED_TABLE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pd_common.h"
#include "pd_msda.h"                         // PD_OK / PD_ERR_*

namespace {

template <typename E>
__device__ __forceinline__ const E *find_entry(const E *table, int count, int64_t wg)
{
  int e = 0;
  while (e + 1 < count && wg >= table[e + 1].wg_begin) ++e;
  return pd_as_global(table + e);
}

template <typename E>
int upload(const E *h, int count, void *table_device, hipStream_t st, const char *what)
{
  if (hipMemcpyAsync(table_device, h, (size_t)count * sizeof(E), hipMemcpyHostToDevice, st) != hipSuccess)
    return pd_set_error(PD_ERR_LAUNCH, "%s: table upload failed", what);
  return PD_OK;
}

// The host side of a grouped entry point up to its launch.  fill(d, i, entry, wg_begin) validates descriptor i and writes Entry i, whose
// first workgroup is wg_begin; it returns the entry's workgroup count, or the (negative) code of the error it has set.  more_ok carries
// the entry point's further pointer arguments into the null check.  Returns the total workgroup count with the table uploaded, 0
// (= PD_OK) when there is nothing to launch, or a negative error code: `if (wgs <= 0) return (int)wgs;` is the caller's whole handling.
template <typename E, typename D, typename F>
int64_t stage_table(const char *name, const D *list, int32_t count, bool more_ok, void *table_host_pinned, void *table_device,
                    hipStream_t st, F fill)
{
  if (count <= 0) return PD_OK;
  if (!list || !more_ok || !table_host_pinned || !table_device) return pd_set_error(PD_ERR_INVALID_ARG, "%s: null pointer", name);
  E *h = reinterpret_cast<E *>(table_host_pinned);
  int64_t wgs = 0;
  for (int i = 0; i < count; ++i) {
    const int64_t n = fill(list[i], i, h[i], wgs);
    if (n < 0) return n;
    wgs += n;
  }
  if (wgs == 0) return PD_OK;
  if (wgs >= INT32_MAX) return pd_set_error(PD_ERR_INVALID_ARG, "%s: %lld workgroups", name, (long long)wgs);
  if (int rc = upload(h, count, table_device, st, name)) return rc;
  return wgs;
}

}  // namespace
#endif
