"""Evaluation branch of SupervisedModel on the device (reference supervised_model.py:201-335, 378-451).

The data mappers of the supervised datasets resize the image, so the output size differs from the size the network saw and the
reference pushes all Q mask-logit maps through two bilinear resizes ([Q, H, W] fp32 each), the object mask, sigmoid, the score multiply
and an arg-max, then computes mask IoUs on the CPU through pycocotools.  With per-pixel-unique post-processing on the GPU this module
runs the whole batch through four launches instead (`inference_fused`):
  pd_masks_resize_u8       ground-truth part masks and object masks at the output size (no float image),
  pd_mask_assign_resized   both interpolations inside the one pass that writes the int16 arg-max map, the object map and, with
                           classification, the class map,
  pd_assign_histogram      won / area / intersection / ground-truth-area counts of every image in one pass,
and ONE device -> host copy of those integer counts (a few KB).  Which queries won a pixel, the IoUs (float64 from exact integers, as
pycocotools computes them), the foreground filter and the merge per class are decided on the host from the counts; the boolean masks
are then cut from the maps on the device.  Plain thresholding, and CPU tensors, take the dense torch route.

Quirks of the reference kept: no area or score filters; `pred_classes` are the matched ground-truth labels in the class-agnostic
case and the predicted labels with classification; when nothing matches, a single all-false mask with label 0 (class-agnostic) or
num_classes (classification)."""
import numpy as np
import torch
import torch.nn.functional as F

from .compat import Instances
from .functions import mask_assign as A
from .functions import pixel_grouping as G
from .inference import mask_iou, sem_seg_postprocess


def _classified(model):
    return not (model.class_agnostic_learning or model.class_agnostic_inference)


def select_queries(model, mask_cls, topk):
    """reference :383-391 / :280-287 -> (scores [K], query index [K], predicted label [K] or None)"""
    scores = mask_cls.float().softmax(-1)[:, :-1]
    if _classified(model):
        nc = model.num_classes
        scores, idx = scores.flatten(0, 1).topk(topk, sorted=False)
        return scores, torch.div(idx, nc, rounding_mode="floor"), idx % nc
    scores = scores.flatten() if model.class_agnostic_learning else scores.topk(1, dim=1)[0].flatten()
    scores, idx = scores.topk(topk, sorted=False)
    return scores, idx, None


def _empty(model, height, width, scores, device):
    """does not contribute to the evaluation (reference :296-301 / :399-403)"""
    label = model.num_classes if _classified(model) else 0
    return (torch.zeros((1, height, width), dtype=torch.bool, device=device), scores.new_zeros(1),
            torch.full((1,), label, dtype=torch.long, device=device))


def instance_inference_dense(model, mask_cls, mask_pred, target_masks, target_object_masks, target_labels, topk):
    """the reference's sequence on dense [K, H, W] tensors"""
    scores, q, labels = select_queries(model, mask_cls, topk)
    mask_pred = mask_pred[q]
    if model.apply_masking_with_object_mask:
        mask_pred = mask_pred * target_object_masks.sum(dim=0, keepdim=True).bool()
    obj_map = mask_pred.max(dim=0)[0] > 0.0
    if model.use_unique_per_pixel_label:
        K = mask_pred.shape[0]
        scoremap = (scores[:, None, None] * mask_pred.sigmoid()).argmax(0)
        ids = (torch.bincount(scoremap.flatten(), minlength=K) > 0).nonzero().flatten()            # scoremap.unique()
        masks = (scoremap[None] == ids[:, None, None]) & obj_map[None]
        scores = scores[ids]
        if labels is not None:                                                                     # merge per predicted class (:327-335)
            labels = labels[ids]
            new_labels = labels.unique()
            member = labels[None, :] == new_labels[:, None]
            masks = (member[:, :, None, None] & masks[None]).any(1)
            scores = torch.where(member, scores[None, :], scores.new_full((), -1.0)).max(dim=1)[0]
            labels = new_labels
    else:
        masks = mask_pred > 0
    if masks.shape[0] == 0 or target_masks.shape[0] == 0:
        return masks[:0], scores[:0], target_labels[:0]
    top1, top1_idx = mask_iou(masks, target_masks).topk(1, dim=1)
    fg = (top1 > 0.001).flatten()
    return masks[fg], scores[fg], (labels[fg] if labels is not None else target_labels[top1_idx.flatten()[fg]])


def _iou_top1(area, inter, gt_area):
    """float64 COCO IoU from integer counts: rows -> (best IoU, its column)"""
    inter = inter.astype(np.float64)
    union = area.astype(np.float64)[:, None] + gt_area.astype(np.float64)[None, :] - inter
    iou = np.where(union > 0, inter / np.maximum(union, 1), 0.0)
    return iou.max(axis=1), iou.argmax(axis=1)


def read_counts(t):
    """the fused route's one device -> host copy per batch (a synchronisation; everything else only enqueues work)"""
    return t.cpu().numpy()


def inference_fused(model, batched_inputs, targets, images, cls_all, logits_all, topk):
    """per-pixel-unique post-processing of a whole batch without dense [Q, H, W] tensors (any output size)"""
    dev = logits_all.device
    pad_hw = tuple(int(s) for s in images.tensor.shape[-2:])
    classified = _classified(model)
    sizes = [(int(inp.get("height", sz[0])), int(inp.get("width", sz[1]))) for inp, sz in zip(batched_inputs, images.image_sizes)]
    resized = G.masks_resize([x for tgt, isz, osz in zip(targets, images.image_sizes, sizes)
                              for x in ((tgt["masks"].bool(), isz, osz), (tgt["object_masks"].bool(), isz, osz))])
    tms = [r[0] for r in resized[0::2]]
    tos = [(r[0][0] if r[0].shape[0] == 1 else r[0].any(0)) for r in resized[1::2]]
    sel, items = [], []
    for cls, low, to, isz, osz in zip(cls_all, logits_all, tos, images.image_sizes, sizes):
        scores, q, labels = select_queries(model, cls, topk)
        sel.append((scores, labels))
        items.append((low[q].float().contiguous(), scores.contiguous(), to if model.apply_masking_with_object_mask else None,
                      labels.to(torch.int32) if classified else None, pad_hw, tuple(isz), osz))
    maps = A.mask_assign_resized(items)
    hist = []
    for (arg, obj, _, clsmap), tm, (scores, _) in zip(maps, tms, sel):
        K = scores.shape[0]
        if classified:
            hist += [(arg, obj, None, K), (clsmap, obj, tm if tm.shape[0] else None, model.num_classes)]
        else:
            hist.append((arg, obj, tm if tm.shape[0] else None, K))
    _, flat = A.assign_histogram(hist, flat=True)
    extra = [s[1] for s in sel] if classified else []
    host = read_counts(torch.cat([flat] + extra))                       # the batch's one device -> host copy: integer counts (+ labels)
    lab_host, pos = host[flat.numel():], 0

    def take(n, G_):
        nonlocal pos
        o = pos
        pos += 2 * n + n * G_ + G_
        return host[o:o + n], host[o + n:o + 2 * n], host[o + 2 * n:o + 2 * n + n * G_].reshape(n, G_), host[o + 2 * n + n * G_:pos]

    results, lo = [], 0
    for (arg, obj, _, clsmap), tm, (scores, labels), tgt, (H, W) in zip(maps, tms, sel, targets, sizes):
        K, Gn = scores.shape[0], tm.shape[0]
        won, area, inter, gt_area = take(K, 0 if classified else Gn)
        ids = np.flatnonzero(won > 0)                                    # scoremap.unique()
        if classified:
            ql = lab_host[lo:lo + K]
            lo += K
            _, area, inter, gt_area = take(model.num_classes, Gn)
            ids_c = np.unique(ql[ids])                                   # classes of the queries that won a pixel, ascending
            rows, member = ids_c, ql[None, ids] == ids_c[:, None]
        else:
            rows = ids
        if Gn and rows.size:
            top1, top1_idx = _iou_top1(area[rows], inter[rows], gt_area)
            fg = top1 > 0.001
        else:
            fg = np.zeros(rows.size, dtype=bool)
        if not fg.any():
            masks, sc, lb = _empty(model, H, W, scores, dev)
        elif classified:
            keep = torch.from_numpy(rows[fg]).to(dev, non_blocking=True)
            m = torch.zeros((int(fg.sum()), K), dtype=torch.bool)
            m[:, ids] = torch.from_numpy(member[fg])
            masks = clsmap[None] == keep[:, None, None].to(torch.int16)
            sc = torch.where(m.to(dev, non_blocking=True), scores[None, :], scores.new_full((), -1.0)).max(dim=1)[0]
            lb = keep
        else:
            keep = torch.from_numpy(rows[fg]).to(dev, non_blocking=True)
            masks = (arg[None] == keep[:, None, None].to(torch.int16)) & obj.bool()[None]
            sc = scores[keep]
            lb = tgt["labels"][torch.from_numpy(top1_idx[fg]).to(dev, non_blocking=True)]
        results.append(_result(masks, sc, lb, tm, tgt["labels"], H, W))
    return results


def _result(masks, scores, labels, tm, gt_labels, H, W):
    r = Instances((H, W))
    r.pred_masks, r.pred_classes, r.scores = masks, labels, scores
    gt = Instances((H, W))
    gt.gt_masks, gt.gt_classes, gt.pred_masks, gt.pred_classes = tm, gt_labels, tm, gt_labels
    return {"predictions": r, "gt_instances": gt, "proposals": r, "gt_masks": gt}


@torch.no_grad()
def supervised_inference(model, batched_inputs, targets, images, outputs):
    """reference :201-248 -> [{"predictions", "gt_instances", "proposals", "gt_masks"}] (predictions is proposals, gt_instances is gt_masks)"""
    logits_all = outputs["pred_masks"]
    if logits_all is None:                                   # decoder ran without dense masks
        from .modeling.transformer_decoder.mask2former_transformer_decoder import materialize_masks
        logits_all = materialize_masks(dict(outputs))["pred_masks"]
    topk = model.test_topk_per_image
    if model.use_unique_per_pixel_label and logits_all.is_cuda:
        if topk > A.MAX_K:
            raise ValueError(f"SupervisedModel: TEST.DETECTIONS_PER_IMAGE = {topk} exceeds the {A.MAX_K} queries per image that "
                             "pd_mask_assign_resized assigns (include/pd_assign.h: PD_ASSIGN_MAX_K)")
        return inference_fused(model, batched_inputs, targets, images, outputs["pred_logits"], logits_all, topk)
    pad_hw = tuple(images.tensor.shape[-2:])
    results = []
    for cls, low, tgt, inp, size in zip(outputs["pred_logits"], logits_all, targets, batched_inputs, images.image_sizes):
        height, width = inp.get("height", size[0]), inp.get("width", size[1])
        dense = F.interpolate(low[None].float(), size=pad_hw, mode="bilinear", align_corners=False)[0]
        dense = sem_seg_postprocess(dense, size, height, width)
        tm = sem_seg_postprocess(tgt["masks"].float(), size, height, width).bool()
        to = sem_seg_postprocess(tgt["object_masks"].float(), size, height, width).bool()
        masks, scores, labels = instance_inference_dense(model, cls, dense, tm, to, tgt["labels"], topk)
        if masks.shape[0] == 0:
            masks, scores, labels = _empty(model, height, width, scores, low.device)
        results.append(_result(masks, scores, labels, tm, tgt["labels"], height, width))
    return results
