/*
 * pd_pparts.h — C-ABI of the panoptic-parts uid decoder of libpd_hip.so.
 *
 * Replaces `panoptic_parts.decode_uids` in front of the reference's Cityscapes-Part ground truth
 * (data/dataset_mappers/cityscapes_part_mapper.py:54-55, data/datasets/register_cityscapes_part.py:57-58).  The published
 * Cityscapes-Panoptic-Parts encoding, restated (panoptic_parts itself is not available to test against: parity UNPINNED):
 *
 *   uid in [0, 99]                  sid = uid            iid = -1                 pid = -1
 *   uid in [100, 99 999]            sid = uid / 1000     iid = uid % 1000         pid = -1
 *   uid in [100 000, 9 999 999]     sid = uid / 100000   iid = (uid / 100) % 1000 pid = uid % 100
 *
 *   pd_pp_decode_uids    uids int32 [numel] -> sids, iids, pids int32 [numel] and part_label uint8 [numel] = pid > 0 ? pid : 0 (the
 *                        reference ignores both -1 and 0).  Every output may be null; null outputs are not computed.  A uid below 0 or
 *                        above 9 999 999 is invalid: every lane that meets one stores 1 to *invalid_flag (plain vector stores of one
 *                        value, no atomic) and writes -1 / -1 / -1 / 0.  The caller clears the flag beforehand; it is never cleared here.
 *                        One streaming pass, 16-byte loads and stores where the pointers are 16-byte aligned (part_label: 4-byte), any
 *                        numel >= 0.
 *
 * `stream` = hipStream_t; returns 0 or PD_ERR_*.
 */
#ifndef PD_PPARTS_H
#define PD_PPARTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_PP_MAX_UID 9999999

int pd_pp_decode_uids(const int32_t *uids, int64_t numel, int32_t *sids, int32_t *iids, int32_t *pids, uint8_t *part_label,
                      int32_t *invalid_flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_PPARTS_H */
