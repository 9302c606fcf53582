"""Host staging shared by the grouped evaluation launches (functions/eval_metrics.py, pixel_grouping.py, mask_assign.py): the
descriptor list of a batch goes through a slot of a pinned ring into one library call, and the small input checks they all make."""
import torch

from .. import lib as _lib

_RINGS = {}


def ptr(t):
    return None if t is None else t.data_ptr()


def require_cuda(family, t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{family}: {what} must be on the GPU (no CPU fallback in partdistillation_amd)")


def as_u8(m, what):
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: bool / uint8 expected, got {m.dtype}")
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def launch(fn, struct, fields, extra, device, table_bytes):
    """fill a host descriptor list, stage it through a pinned ring slot and call fn(list, count, *extra, pinned, device table, stream);
    table_bytes names the library's size query of the kernel family"""
    L = _lib.load()
    arr = (struct * len(fields))()
    for d, f in zip(arr, fields):
        for k, v in f.items():
            setattr(d, k, v)
    nbytes = int(getattr(L, table_bytes)(len(fields)))
    cap = 1 << max(8, (nbytes - 1).bit_length())
    ring = _RINGS.get(cap)
    if ring is None:
        from .fused import PinnedRing
        ring = _RINGS[cap] = PinnedRing(cap, torch.uint8, pin=True)
    tdev = torch.empty(cap, dtype=torch.uint8, device=device)
    host = ring.acquire()
    rc = getattr(L, fn)(arr, len(fields), *extra, host.data_ptr(), tdev.data_ptr(), _lib.current_stream())
    ring.release()
    _lib.check(rc)
