"""Panoptic-parts uid maps on the device (include/pd_pparts.h, csrc/panoptic_parts.hip): `panoptic_parts.decode_uids` of the reference's
Cityscapes-Part ground truth (cityscapes_part_mapper.py:54-55) restated from the published Cityscapes-Panoptic-Parts encoding.
panoptic_parts itself is not available to test against: parity with it is UNPINNED.  GPU only; there is no fallback."""
import torch

from .. import lib as _lib

OUTPUTS = ("sids", "iids", "pids", "part_label")
MAX_UID = 9999999                # PD_PP_MAX_UID


class DecodedUids(dict):
    """the requested outputs by name (int32 [H, W]; part_label uint8 [H, W]) and the device flag an invalid uid has set.  Nothing has
    been read back when this is returned: `check()` reads the flag, best right after a blocking read the caller does anyway."""

    def __init__(self, outputs, flag):
        super().__init__(outputs)
        self.flag = flag

    def check(self):
        if int(self.flag.item()):
            raise ValueError(f"decode_uids: the map holds a uid outside [0, {MAX_UID}], the range of the panoptic-parts encoding")
        return self


def decode_uids(uids, want=OUTPUTS):
    """uids int32 [H, W] on the GPU -> DecodedUids of the outputs named in `want`: sids, iids, pids (-1 where the uid has none) and
    part_label = pid where pid > 0, else 0.  One launch, no synchronisation; an invalid uid becomes a ValueError at `.check()`."""
    if not (torch.is_tensor(uids) and uids.is_cuda):
        raise RuntimeError("pd_pp_decode_uids runs on the GPU only (no CPU fallback in partdistillation_amd)")
    if uids.dim() != 2 or uids.dtype != torch.int32:
        raise ValueError(f"decode_uids: int32 [H, W] expected, got {uids.dtype} {tuple(uids.shape)}")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or not set(want) <= set(OUTPUTS):
        raise ValueError(f"decode_uids: want = {want}: distinct names out of {OUTPUTS} expected")
    uids = uids.contiguous()
    out = {k: torch.empty(uids.shape, dtype=torch.uint8 if k == "part_label" else torch.int32, device=uids.device) for k in want}
    flag = torch.zeros(1, dtype=torch.int32, device=uids.device)
    with torch.cuda.device(uids.device):
        _lib.check(_lib.load().pd_pp_decode_uids(uids.data_ptr(), uids.numel(), *(out[k].data_ptr() if k in out else None for k in OUTPUTS),
                                                 flag.data_ptr(), _lib.current_stream()))
    return DecodedUids(out, flag)
