"""Per-pixel mask assignment at a resized output and its histogram on the device (include/pd_assign.h, csrc/mask_assign_resized.hip).
Each function is ONE launch for all images of a batch (descriptor table staged through the pinned ring of functions/grouped_launch.py)
and reads nothing back to the host."""
from functools import partial

import torch

from .. import lib as _lib
from .grouped_launch import as_u8, launch_fields, require_cuda

MAX_K, MAX_KEYS, MAX_GT = (_lib.const(n) for n in ("PD_ASSIGN_MAX_K", "PD_ASSIGN_MAX_KEYS", "PD_ASSIGN_MAX_GT"))
MAX_Q = _lib.const("PD_ASSIGN_MAX_Q")
_cuda = partial(require_cuda, "pd_assign")
_launch = partial(launch_fields, table_bytes="pd_assign_table_bytes")


PdAssignResized = _lib.struct("PdAssignResized")
PdAssignPairs = _lib.struct("PdAssignPairs")
PdAssignHistogram = _lib.struct("PdAssignHistogram")


def mask_assign_resized(items):
    """items: [(logits fp32 [K, h, w], scores fp32 [K], object bool / uint8 [H, W] or None, cls_of_query int32 [K] or None, (Hp, Wp),
    (Hi, Wi), (H, W))] -> [(arg int16 [H, W], obj uint8 [H, W], positive int32 [K], cls int16 [H, W] or None)].
    v_k = logits_k interpolated to (Hp, Wp), cropped to (Hi, Wi), interpolated to (H, W), times (object != 0);
    arg = argmax_k scores[k] * sigmoid(v_k), obj = max_k v_k > 0, positive[k] = #(v_k > 0), cls = obj ? cls_of_query[arg] : -1."""
    if not items:
        return []
    dev = items[0][0].device
    for it in items:
        _cuda(it[0], "logits")
    ktot = sum(int(it[0].shape[0]) for it in items)
    positive = torch.zeros(max(ktot, 1), dtype=torch.int32, device=dev)
    fields, keep, out, off = [], [], [], 0
    for logits, scores, obj_in, coq, (Hp, Wp), (Hi, Wi), (H, W) in items:
        if logits.dtype != torch.float32 or logits.dim() != 3 or scores.dtype != torch.float32 or scores.numel() != logits.shape[0]:
            raise ValueError(f"mask_assign_resized: fp32 logits [K, h, w] and fp32 scores [K] expected, got {logits.dtype} {tuple(logits.shape)}, "
                             f"{scores.dtype} {tuple(scores.shape)}")
        K, h, w = (int(s) for s in logits.shape)
        H, W = int(H), int(W)
        logits, scores = logits.contiguous(), scores.contiguous()
        _cuda(scores, "scores")
        o8 = None
        if obj_in is not None:
            _cuda(obj_in, "object mask")
            o8 = as_u8(obj_in, "mask_assign_resized: object mask")
            if tuple(o8.shape) != (H, W):
                raise ValueError(f"mask_assign_resized: object mask {tuple(o8.shape)} is not at the output size {(H, W)}")
        if coq is not None:
            _cuda(coq, "cls_of_query")
            if coq.dtype != torch.int32 or coq.numel() != K:
                raise ValueError(f"mask_assign_resized: cls_of_query must be int32 [{K}], got {coq.dtype} {tuple(coq.shape)}")
            coq = coq.contiguous()
        arg = torch.empty((H, W), dtype=torch.int16, device=dev)
        obj = torch.empty((H, W), dtype=torch.uint8, device=dev)
        cls = torch.empty((H, W), dtype=torch.int16, device=dev) if coq is not None else None
        keep += [logits, scores, o8, coq]
        out.append((arg, obj, positive[off:off + K], cls))
        fields.append(dict(logits=logits.data_ptr(), scores=scores.data_ptr(), object=None if o8 is None else o8.data_ptr(),
                           cls_of_query=None if coq is None else coq.data_ptr(), arg=arg.data_ptr(), obj=obj.data_ptr(),
                           positive=positive.data_ptr() + 4 * off, cls=None if cls is None else cls.data_ptr(), K=K, h=h, w=w, Hp=int(Hp),
                           Wp=int(Wp), Hi=int(Hi), Wi=int(Wi), H=H, W=W))
        off += K
    _launch("pd_mask_assign_resized", PdAssignResized, fields, (), dev)
    return out


def pair_assign_resized(items):
    """mask_assign_resized for (query, class) pairs that share queries, without the gathered [K, h, w] copy.
    items: [(logits fp32 [Q, h, w], pair_query int32 [K] with values in [0, Q) (the caller's contract), scores fp32 [K],
    object bool / uint8 [H, W] or None, cls_of_pair int32 [K] or None, (Hp, Wp), (Hi, Wi), (H, W))] ->
    [(arg int16 [H, W] (pair index), obj uint8 [H, W], positive int32 [K], cls int16 [H, W] or None)], bit-identical to
    mask_assign_resized on logits[pair_query]."""
    if not items:
        return []
    dev = items[0][0].device
    for it in items:
        _cuda(it[0], "logits")
    ktot = sum(int(it[1].numel()) for it in items)
    positive = torch.zeros(max(ktot, 1), dtype=torch.int32, device=dev)
    fields, keep, out, off = [], [], [], 0
    for logits, pq, scores, obj_in, cop, (Hp, Wp), (Hi, Wi), (H, W) in items:
        if logits.dtype != torch.float32 or logits.dim() != 3 or scores.dtype != torch.float32 or scores.dim() != 1:
            raise ValueError(f"pair_assign_resized: fp32 logits [Q, h, w] and fp32 scores [K] expected, got {logits.dtype} {tuple(logits.shape)}, "
                             f"{scores.dtype} {tuple(scores.shape)}")
        Q, h, w = (int(s) for s in logits.shape)
        K, H, W = int(scores.numel()), int(H), int(W)
        _cuda(scores, "scores")
        _cuda(pq, "pair_query")
        if pq.dtype != torch.int32 or pq.dim() != 1 or pq.numel() != K:
            raise ValueError(f"pair_assign_resized: pair_query must be int32 [{K}], got {pq.dtype} {tuple(pq.shape)}")
        logits, scores, pq = logits.contiguous(), scores.contiguous(), pq.contiguous()
        o8 = None
        if obj_in is not None:
            _cuda(obj_in, "object mask")
            o8 = as_u8(obj_in, "pair_assign_resized: object mask")
            if tuple(o8.shape) != (H, W):
                raise ValueError(f"pair_assign_resized: object mask {tuple(o8.shape)} is not at the output size {(H, W)}")
        if cop is not None:
            _cuda(cop, "cls_of_pair")
            if cop.dtype != torch.int32 or cop.numel() != K:
                raise ValueError(f"pair_assign_resized: cls_of_pair must be int32 [{K}], got {cop.dtype} {tuple(cop.shape)}")
            cop = cop.contiguous()
        arg = torch.empty((H, W), dtype=torch.int16, device=dev)
        obj = torch.empty((H, W), dtype=torch.uint8, device=dev)
        cls = torch.empty((H, W), dtype=torch.int16, device=dev) if cop is not None else None
        keep += [logits, scores, pq, o8, cop]
        out.append((arg, obj, positive[off:off + K], cls))
        fields.append(dict(logits=logits.data_ptr(), pair_query=pq.data_ptr(), scores=scores.data_ptr(),
                           cls_of_pair=None if cop is None else cop.data_ptr(), object=None if o8 is None else o8.data_ptr(),
                           arg=arg.data_ptr(), obj=obj.data_ptr(), positive=positive.data_ptr() + 4 * off,
                           cls=None if cls is None else cls.data_ptr(), K=K, Q=Q, h=h, w=w, Hp=int(Hp), Wp=int(Wp), Hi=int(Hi), Wi=int(Wi),
                           H=H, W=W))
        off += K
    _launch("pd_pair_assign_resized", PdAssignPairs, fields, (), dev)
    return out


def assign_histogram(items, flat=False):
    """items: [(key int16 [H, W] (arg or cls), obj uint8 / bool [H, W], gt bool / uint8 [G, H, W] or None, n)] ->
    [(won int64 [n], area int64 [n], inter int64 [n, G], gt_area int64 [G])]: won[k] = #(key == k), area[k] = #(key == k & obj),
    inter[k, j] = #(key == k & obj & gt_j), gt_area[j] = #gt_j.  Keys outside [0, n) only count in gt_area.  G may be 0.
    flat=True also returns the one int64 tensor all results are views of (per item: won, area, inter, gt_area side by side), for a
    single copy to the host."""
    if not items:
        return ([], None) if flat else []
    dev = items[0][0].device
    layout, tot = [], 0
    for key, obj, gt, n in items:
        _cuda(key, "key map")
        G = 0 if gt is None else int(gt.shape[0])
        n = int(n)
        layout.append((n, G, tot))
        tot += 2 * n + n * G + G
    counts = torch.zeros(max(tot, 1), dtype=torch.int64, device=dev)
    fields, keep, out = [], [], []
    for (key, obj, gt, _), (n, G, o) in zip(items, layout):
        if key.dtype != torch.int16 or key.dim() != 2 or tuple(obj.shape) != tuple(key.shape):
            raise ValueError(f"assign_histogram: int16 key map [H, W] and an object map of its size expected, got {key.dtype} {tuple(key.shape)}, "
                             f"{tuple(obj.shape)}")
        _cuda(obj, "object map")
        key, o8 = key.contiguous(), as_u8(obj, "assign_histogram: object map")
        g8 = None
        if G:
            _cuda(gt, "gt masks")
            if tuple(gt.shape[1:]) != tuple(key.shape):
                raise ValueError(f"assign_histogram: gt masks {tuple(gt.shape)} do not match the map {tuple(key.shape)}")
            g8 = as_u8(gt, "assign_histogram: gt masks")
        keep += [key, o8, g8]
        base = counts.data_ptr() + 8 * o
        won, area = counts[o:o + n], counts[o + n:o + 2 * n]
        inter, gt_area = counts[o + 2 * n:o + 2 * n + n * G].view(n, G), counts[o + 2 * n + n * G:o + 2 * n + n * G + G]
        out.append((won, area, inter, gt_area))
        fields.append(dict(key=key.data_ptr(), obj=o8.data_ptr(), gt=None if g8 is None else g8.data_ptr(), won=base, area=base + 8 * n,
                           inter=base + 16 * n if G else None, gt_area=base + 8 * (2 * n + n * G) if G else None, n=n, G=G, hw=key.numel()))
    _launch("pd_assign_histogram", PdAssignHistogram, fields, (), dev)
    return (out, counts[:tot]) if flat else out
