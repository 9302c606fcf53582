"""Label maps and boolean masks of resized evaluation images on the device (include/pd_grouping.h, csrc/pixel_grouping.hip).  Each
function is ONE launch for all images of a batch (descriptor table staged through the pinned ring of functions/grouped_launch.py) and
reads nothing back to the host."""
from functools import partial

import torch

from .. import lib as _lib
from .grouped_launch import as_u8, launch_fields, require_cuda

MAX_K = _lib.const("PD_GROUPING_MAX_K")
_cuda = partial(require_cuda, "pd_grouping")
_launch = partial(launch_fields, table_bytes="pd_grouping_table_bytes")


PdGroupLabels = _lib.struct("PdGroupLabels")
PdMaskResize = _lib.struct("PdMaskResize")


def scores_argmax_resized(items):
    """items: [(scores fp32 [K, h, w], mask bool / uint8 [H, W], (Hp, Wp), (Hi, Wi))] -> ([labels uint8 [H, W]], counts int32 [B, Kmax + 1]).
    labels = mask ? 1 + argmax_k of scores_k interpolated to (Hp, Wp), cropped to (Hi, Wi) and interpolated to (H, W) : 0;
    counts[b, l] = pixels of image b with label l (columns past K_b stay 0)."""
    if not items:
        return [], None
    dev = items[0][0].device
    kmax = max(int(s.shape[0]) for s, _, _, _ in items)
    fields, keep, labels = [], [], []
    for s, m, _, _ in items:
        _cuda(s, "scores")
        _cuda(m, "mask")
    counts = torch.zeros((len(items), kmax + 1), dtype=torch.int32, device=dev)
    for b, (s, m, (Hp, Wp), (Hi, Wi)) in enumerate(items):
        if s.dtype != torch.float32 or s.dim() != 3 or not 1 <= s.shape[0] <= MAX_K or m.dim() != 2:
            raise ValueError(f"scores_argmax_resized: fp32 scores [K <= {MAX_K}, h, w] and a mask [H, W] expected, got {s.dtype} {tuple(s.shape)}, "
                             f"{tuple(m.shape)}")
        s, m8 = s.contiguous(), as_u8(m, "scores_argmax_resized: mask")
        H, W = m8.shape
        out = torch.empty((H, W), dtype=torch.uint8, device=dev)
        keep += [s, m8]
        labels.append(out)
        fields.append(dict(scores=s.data_ptr(), mask=m8.data_ptr(), labels=out.data_ptr(), counts=counts[b].data_ptr(), K=s.shape[0],
                           h=s.shape[1], w=s.shape[2], Hp=int(Hp), Wp=int(Wp), Hi=int(Hi), Wi=int(Wi), H=H, W=W))
    _launch("pd_scores_argmax_resized_u8", PdGroupLabels, fields, (), dev)
    return labels, counts


def masks_resize(items):
    """items: [(masks bool / uint8 [n, Hp, Wp], (Hi, Wi), (H, W))] -> [(resized bool [n, H, W], area int64 [n])]:
    `sem_seg_postprocess(masks.float(), (Hi, Wi), H, W).bool()` without the float image.  n may be 0."""
    if not items:
        return []
    dev = items[0][0].device
    fields, keep, out, ntot = [], [], [], 0
    for m, _, _ in items:
        _cuda(m, "masks")
        ntot += m.shape[0]
    area = torch.zeros(max(ntot, 1), dtype=torch.int64, device=dev)
    off = 0
    for m, (Hi, Wi), (H, W) in items:
        if m.dim() != 3:
            raise ValueError(f"masks_resize: masks [n, Hp, Wp] expected, got {tuple(m.shape)}")
        m8 = as_u8(m, "masks_resize: masks")
        n, Hp, Wp = m8.shape
        dst = torch.empty((n, int(H), int(W)), dtype=torch.uint8, device=dev)
        keep.append(m8)
        out.append((dst.view(torch.bool), area[off:off + n]))
        fields.append(dict(src=m8.data_ptr() if n else None, dst=dst.data_ptr() if n else None, area=area.data_ptr() + 8 * off, n=n, Hp=Hp, Wp=Wp,
                           Hi=int(Hi), Wi=int(Wi), H=int(H), W=int(W)))
        off += n
    _launch("pd_masks_resize_u8", PdMaskResize, fields, (), dev)
    return out
