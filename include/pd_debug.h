/*
 * pd_debug.h — development knobs of libpd_hip.so.  NOT part of the product contract: tools/, the benchmarks' A/B switches and the tests
 * that force a kernel variant use them; the product never calls them (lib.load() applies the PD_DEBUG_SET environment variable, which
 * is a development switch too).  They are declared here so that every exported symbol has a prototype the binding is derived from;
 * their keys and their meaning change without an ABI bump.
 */
#ifndef PD_DEBUG_H
#define PD_DEBUG_H

#include <stdint.h>

#include "pd_igemm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* set / read an experiment knob by name (csrc/common.hip lists the keys); PD_ERR_INVALID_ARG for an unknown key.  pd_debug_get
 * knows only the knobs that tests change and have to put back. */
int pd_debug_set(const char *key, int value);
int pd_debug_get(const char *key, int *value);

/* `iters` back-to-back launches of one problem between two events: *us <- average microseconds per launch.  Synchronises. */
int pd_igemm_bf16_time(const PdIgemm *p, void *workspace, int64_t workspace_bytes, int iters, float *us, void *stream);
int pd_wgrad_bf16_time(const PdWgrad *p, void *workspace, int64_t workspace_bytes, int iters, float *us, void *stream);

/* stamps of the traced f16x2 GEMM variants (tools/debug/kpc_trace.py): dst[2 * 64 * 8] <- the device-side trace buffer.  Synchronises. */
int pd_debug_read_kpc_trace(unsigned long long *dst);

/* what pd_debug_set("wgrad_xcd" / "wgrad_fast") calls: the two knobs live in device memory (csrc/gemm_x3.hip) */
void pd_dbg_set_wgrad_xcd(int v);
void pd_dbg_set_wgrad_fast(int v);

#ifdef __cplusplus
}
#endif
#endif /* PD_DEBUG_H */
