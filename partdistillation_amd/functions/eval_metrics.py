"""Evaluation counters on the device (include/pd_eval.h): bit planes of masks, pairwise intersections, label-map confusion tables
and the greedy cover of the box-proposal recall.  Every result is an exact integer count; each function is one launch for a whole
batch of images (a descriptor table staged through a pinned ring), and none reads anything back to the host.

Bit planes are int64 tensors [n, ceil(H*W / 64)] holding the 64-bit words of pd_eval.h (pixel q = bit q % 64 of word q / 64)."""
from functools import partial

import torch

from .. import lib as _lib
from .grouped_launch import as_u8, launch_fields, ptr, require_cuda

LIMITS = (1, 10, 50, 100, 200)            # AR@k of the proposal evaluator
MAX_ROWS, MAX_GT = _lib.const("PD_EVAL_MAX_ROWS"), _lib.const("PD_EVAL_MAX_GT")
_cuda = partial(require_cuda, "pd_eval")
_launch = partial(launch_fields, table_bytes="pd_eval_table_bytes")


PdEvalMaskSet = _lib.struct("PdEvalMaskSet")
PdEvalPairs = _lib.struct("PdEvalPairs")
PdEvalConfusion = _lib.struct("PdEvalConfusion")
PdEvalRecall = _lib.struct("PdEvalRecall")


def words_of(hw):
    return (int(hw) + 63) // 64


def pack_masks(mask_sets):
    """[masks [n_i, H_i, W_i] (or [n_i, HW_i]) bool / uint8 on the device] -> [(bits int64 [n_i, words_i], area int64 [n_i])], one launch"""
    if not mask_sets:
        return []
    dev = mask_sets[0].device
    flat, layout, wtot, ntot = [], [], 0, 0
    for m in mask_sets:
        _cuda(m, "masks")
        if m.dtype not in (torch.bool, torch.uint8) or m.dim() < 1:
            raise ValueError(f"pack_masks: bool / uint8 masks [n, ...] expected, got {m.dtype} {tuple(m.shape)}")
        n = m.shape[0]
        hw = m[0].numel() if n else int(torch.tensor(m.shape[1:]).prod())
        if hw <= 0:
            raise ValueError("pack_masks: empty masks")
        flat.append(as_u8(m, "pack_masks").reshape(n, hw))
        layout.append((n, hw, wtot, ntot))
        wtot += n * words_of(hw)
        ntot += n
    bits = torch.empty(max(wtot, 1), dtype=torch.int64, device=dev)
    area = torch.zeros(max(ntot, 1), dtype=torch.int64, device=dev)
    fields = [dict(masks=ptr(m), bits=bits.data_ptr() + 8 * wo, area=area.data_ptr() + 8 * no, n=n, hw=hw)
              for m, (n, hw, wo, no) in zip(flat, layout)]
    _launch("pd_eval_pack_grouped", PdEvalMaskSet, fields, (), dev)
    return [(bits[wo:wo + n * words_of(hw)].view(n, words_of(hw)), area[no:no + n]) for n, hw, wo, no in layout]


def intersections(items):
    """[(a bits [*, words], rows int64 [p] or None, b bits [g, words])] -> [inter int64 [p, g]]: popcount(a[rows[r]] & b[j]), one launch.
    p = len(rows) (a.shape[0] without rows) >= 1, 1 <= g <= 64."""
    if not items:
        return []
    dev = items[0][0].device
    layout, tot = [], 0
    for a, rows, b in items:
        _cuda(a, "bit planes")
        p = a.shape[0] if rows is None else rows.numel()
        g = b.shape[0]
        if a.dtype != torch.int64 or b.dtype != torch.int64 or a.shape[1] != b.shape[1] or not a.is_contiguous() or not b.is_contiguous():
            raise ValueError("intersections: contiguous int64 bit planes of one width expected")
        if rows is not None and (rows.dtype != torch.int64 or not rows.is_contiguous()):
            raise ValueError("intersections: rows must be a contiguous int64 tensor")
        if p < 1 or not 1 <= g <= MAX_GT:
            raise ValueError(f"intersections: p = {p} >= 1 and 1 <= g = {g} <= {MAX_GT} required")
        layout.append((p, g, tot))
        tot += p * g
    inter = torch.zeros(tot, dtype=torch.int64, device=dev)
    fields = [dict(a=a.data_ptr(), rows=ptr(rows), b=b.data_ptr(), inter=inter.data_ptr() + 8 * o, p=p, g=g, words=a.shape[1])
              for (a, rows, b), (p, g, o) in zip(items, layout)]
    _launch("pd_eval_intersect_grouped", PdEvalPairs, fields, (), dev)
    return [inter[o:o + p * g].view(p, g) for p, g, o in layout]


def confusion_add(items, n, conf):
    """conf int64 [S, n + 1, n + 1] += the (pred label, gt label) pixel counts of every image, one launch.
    items: [(pred bits [P, words], pred classes int64 [P], gt bits [G, words], gt classes int64 [G], slot int64 (device, >= 1 element:
    the first is the image's row of conf), hw)].  Labels: the class of the last mask covering a pixel, n where none does."""
    if not items:
        return conf
    if conf.dtype != torch.int64 or conf.dim() != 3 or conf.shape[1:] != (n + 1, n + 1) or not conf.is_contiguous():
        raise ValueError(f"confusion_add: conf must be contiguous int64 [S, {n + 1}, {n + 1}]")
    _cuda(conf, "conf")
    fields, slots = [], []
    for pb, pc, gb, gc, slot, hw in items:
        for t in (pb, pc, gb, gc):
            if t.dtype != torch.int64 or not t.is_contiguous():
                raise ValueError("confusion_add: contiguous int64 bit planes and classes expected")
        if pb.shape[0] != pc.numel() or gb.shape[0] != gc.numel() or (pb.shape[0] and pb.shape[1] != words_of(hw)) \
                or (gb.shape[0] and gb.shape[1] != words_of(hw)):
            raise ValueError("confusion_add: planes / classes / hw disagree")
        if slot.dtype != torch.int64 or slot.numel() < 1 or not slot.is_cuda:
            raise ValueError("confusion_add: slot must be a device int64 tensor")
        slots.append(slot.reshape(-1)[:1].contiguous())              # (kept alive until the launch is enqueued)
        fields.append(dict(pred_bits=pb.data_ptr(), pred_cls=pc.data_ptr(), gt_bits=gb.data_ptr(), gt_cls=gc.data_ptr(),
                           slot=slots[-1].data_ptr(), pred_n=pb.shape[0], gt_n=gb.shape[0], hw=hw))
    _launch("pd_eval_confusion_grouped", PdEvalConfusion, fields, (n, conf.data_ptr(), conf.shape[0]), conf.device)
    return conf


def thresholds(device):
    """the reference's IoU thresholds, float32 as torch.arange makes them"""
    t = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)
    if torch.device(device).type == "cuda":
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def recall_add(items, thr, hits, num_pos):
    """greedy cover of the box-proposal recall, one workgroup per image, one launch: hits int64 [5, 10] and num_pos int64 [5] (limits
    1, 10, 50, 100, 200) += the counts of every image.  items: [(inter int64 [p, g] rows in score order, rows int64 [p] or None,
    area_p int64, area_g int64 [g])], 1 <= p <= 200, 1 <= g <= 64; thr float32 [10] on the device."""
    if not items:
        return
    if hits.shape != (len(LIMITS), 10) or num_pos.shape != (len(LIMITS),) or hits.dtype != torch.int64 or num_pos.dtype != torch.int64 \
            or thr.dtype != torch.float32 or thr.numel() != 10 or not (hits.is_contiguous() and num_pos.is_contiguous() and thr.is_contiguous()):
        raise ValueError("recall_add: hits int64 [5, 10], num_pos int64 [5], thresholds float32 [10] expected")
    _cuda(hits, "hits")
    fields = []
    for inter, rows, area_p, area_g in items:
        p, g = inter.shape
        if not (1 <= p <= MAX_ROWS and 1 <= g <= MAX_GT) or inter.dtype != torch.int64 or not inter.is_contiguous() \
                or area_g.numel() != g or (rows is not None and rows.numel() != p):
            raise ValueError(f"recall_add: inter int64 [p <= {MAX_ROWS}, g <= {MAX_GT}] with matching rows / areas expected")
        fields.append(dict(inter=inter.data_ptr(), rows=ptr(rows), area_p=area_p.data_ptr(), area_g=area_g.data_ptr(), p=p, g=g))
    _launch("pd_eval_recall_grouped", PdEvalRecall, fields, (thr.data_ptr(), hits.data_ptr(), num_pos.data_ptr()), hits.device)
