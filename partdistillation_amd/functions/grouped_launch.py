"""Host staging shared by every "N problems, one launch" family — the evaluation launches (functions/eval_metrics.py, pixel_grouping.py,
mask_assign.py) and the training-side tables (the grouped weight gradients of gemm.py, smallgemm.py and conv_bf16.py, the filter transposes,
weight packs and MX quantisations): the descriptor list goes through a slot of a pinned ring into one library call.  The rules a grouped
launch must keep inside a recorded region (cmdbuf.py) are written here once: the device table and the workspace are allocated per call
(inside a recording that is arena memory), the rings are created under host_ops(), and every address a descriptor holds goes through
require_stable(); the caller's part is a fresh descriptor array per call, which the recording keeps by reference.  Also the small input
checks the evaluation faces all make."""
import torch

from .. import cmdbuf
from .. import lib as _lib

_RINGS = {}                  # pinned staging rings by power-of-two capacity in bytes, shared by all families
_WS = {}                     # fp32 workspaces by (family, device index, raw stream)


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


def fill(struct, fields):
    """one dict of field values per problem -> the ctypes descriptor array"""
    arr = (struct * len(fields))()
    for d, f in zip(arr, fields):
        for k, v in f.items():
            setattr(d, k, v)
    return arr


def require_stable(named_ptrs, what):
    """(address or tensor or None, name) pairs about to be written into a descriptor table: inside a recorded region each must be a
    persistent address (cmdbuf.require_stable; outside a recording it returns at once)"""
    if cmdbuf.active() is None:
        return
    for p, name in named_ptrs:
        if p is not None:
            cmdbuf.require_stable(p if isinstance(p, int) else p.data_ptr(), f"{what} {name}")


def workspace(family, device, need_floats, floor):
    """fp32 scratch of need_floats for a launch on the current stream of `device`: inside a recorded region a buffer of the region's own
    (arena memory), otherwise one persistent buffer per (family, device, stream) that grows on demand and never starts below `floor` floats —
    consecutive launches on a stream use it in order"""
    if cmdbuf.active() is not None:
        return torch.empty(max(need_floats, 1), dtype=torch.float32, device=device)
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (family, idx, torch._C._cuda_getCurrentRawStream(idx))
    ws = _WS.get(key)
    if ws is None or ws.numel() < need_floats:
        ws = _WS[key] = torch.empty(max(need_floats, floor), dtype=torch.float32, device=device)
    return ws


def launch(fn, descs, count, *, table_bytes, pre=(), post=(), device):
    """stage the first `count` descriptors of the ctypes array `descs` through a pinned ring slot and call
    fn(descs, count, *pre, pinned table, device table, *post, stream) on the current stream of `device`; fn and table_bytes name the
    library's entry point and the size query of its table"""
    with torch.cuda.device(device):
        L = _lib.load()
        nbytes = int(getattr(L, table_bytes)(count))
        cap = 1 << max(8, (nbytes - 1).bit_length())
        ring = _RINGS.get(cap)
        if ring is None:
            from .fused import PinnedRing
            with cmdbuf.host_ops():
                ring = _RINGS[cap] = PinnedRing(cap, torch.uint8, pin=True)
        tdev = torch.empty(cap, dtype=torch.uint8, device=device)
        host = ring.acquire()
        rc = getattr(L, fn)(descs, count, *pre, host.data_ptr(), tdev.data_ptr(), *post, _lib.current_stream())
        ring.release()
    _lib.check(rc)


def launch_fields(fn, struct, fields, extra, device, table_bytes):
    """launch() for callers that describe their problems as dicts of field values"""
    launch(fn, fill(struct, fields), len(fields), table_bytes=table_bytes, pre=extra, device=device)
