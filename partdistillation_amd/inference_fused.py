"""Per-pixel-unique evaluation branches of inference.py without dense [K, H, W] stacks: PartDistillationModel
(`pd_fused`), PartRankingModel (labelling modes `rank_label_fused`, mode "cluster" `rank_cluster_fused`) and ProposalModel with a
resized output (`proposal_fused`).  Each handles a whole batch like inference_supervised.inference_fused:
  pd_masks_resize_u8        ground-truth part masks and object masks at the output size,
  pd_pair_assign_resized    the arg-max map over the K selected (query, class) pairs straight from the decoder's [Q, h, w] logits (no
                            gathered copy; a query shared by several pairs is interpolated once), the object map and the class map
                            (ProposalModel's K distinct queries go through pd_mask_assign_resized),
  pd_assign_histogram       won / area / intersection / ground-truth-area counts,
and ONE device -> host copy (`read_counts`) of the integer counts, the pairs' labels and the bits of their scores.  Which pairs won a
pixel, the merge per class, the area-ratio / score filters, the IoUs (float64 from exact integers) and the foreground match are decided
on the host by the pure functions below; the boolean masks are then cut from the maps and the scores gathered on the device.

A route answers None when a limit of the kernels does not hold (K > PD_ASSIGN_MAX_K, Q > PD_ASSIGN_MAX_Q, G > PD_ASSIGN_MAX_GT, more
classes than PD_ASSIGN_MAX_KEYS): the caller then takes the dense route, which also serves plain thresholding and CPU tensors.
PD_FUSED_INFERENCE=0 forces the dense route in every branch of inference.py, ProposalModel's pd_mask_assign route included (tools,
A/B runs); it is read at every call."""
import os

import numpy as np
import torch

from . import inference as D
from .compat import Instances
from .functions import mask_assign as A
from .functions import pixel_grouping as G
from .inference_supervised import _iou_top1


def enabled():
    return os.environ.get("PD_FUSED_INFERENCE", "1") != "0"


def read_counts(t):
    """a fused route's one device -> host copy per batch (a synchronisation; everything else only enqueues work)"""
    return t.cpu().numpy()


# ================================================================================================ host decisions (pure numpy)
def filter_rows(area, obj_area, scores, min_ratio, min_score):
    """inference._filter on counts: area int64 [P], obj_area int, scores fp32 [P] -> kept row indices"""
    keep = np.arange(scores.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        valid = area.astype(np.float64) / np.float64(obj_area) > min_ratio
    if valid.any():
        keep = keep[valid]
    valid = scores[keep] > np.float32(min_score)              # torch compares an fp32 tensor with a Python number in fp32
    if valid.any():
        keep = keep[valid]
    return keep


def match_rows(area, inter, gt_area, threshold):
    """rows whose best float64 IoU with a ground-truth mask exceeds threshold -> (bool [P], index of the best mask int64 [P])"""
    if area.shape[0] == 0 or gt_area.shape[0] == 0:
        return np.zeros(area.shape[0], dtype=bool), np.zeros(area.shape[0], dtype=np.int64)
    top1, top1_idx = _iou_top1(area, inter, gt_area)
    return top1 > threshold, top1_idx.astype(np.int64)


def decide_queries(won, area, scores, min_ratio, min_score):
    """class-agnostic proposals (inference.instance_inference_dense / _rank_unique_assignment, per-pixel-unique): the queries that won a
    pixel, ascending, through the two filters.  won, area int64 [K] (area[k] = #(arg == k & obj)), scores fp32 [K] -> query indices"""
    ids = np.flatnonzero(won > 0)                                         # scoremap.unique()
    return ids[filter_rows(area[ids], area.sum(), scores[ids], min_ratio, min_score)]


def decide_classes(won, labels, scores, area_c, inter_c, gt_area, min_ratio, min_score, fg_threshold, limit="PD_ASSIGN_MAX_KEYS"):
    """inference._unique_assignment_with_classes (per-pixel-unique) and the foreground match that follows it, on counts.
    won int64 [K]: pixels won by every (query, class) pair; labels int64 [K], scores fp32 [K] of the pairs; area_c int64 [n],
    inter_c int64 [n, G], gt_area int64 [G]: the histogram of the class map.  -> (classes int64 [P] ascending, the pair that gives each
    class its score int64 [P], index of each class's best ground-truth mask int64 [P])"""
    n = area_c.shape[0]
    if labels.size and (int(labels.max()) >= n or int(labels.min()) < 0):
        raise ValueError(f"part label {int(labels.max() if labels.max() >= n else labels.min())} lies outside [0, {n}): the class histogram "
                         f"holds {n} keys ({limit})")
    ids = np.flatnonzero(won > 0)                                         # scoremap.unique()
    lab = labels[ids]
    classes = np.unique(lab)                                              # ascending
    best = np.zeros(classes.shape[0], dtype=np.int64)
    for i, c in enumerate(classes):
        members = ids[lab == c]
        best[i] = members[np.argmax(scores[members])]
    area = area_c[classes]
    keep = filter_rows(area, area.sum(), scores[best], min_ratio, min_score)   # every object pixel carries the class of a winning pair
    classes, best, area = classes[keep], best[keep], area[keep]
    fg, gt_idx = match_rows(area, inter_c[classes], gt_area, fg_threshold)
    return classes[fg], best[fg], gt_idx[fg]


# ================================================================================================ device side
class _Counts:
    """the one host array of a batch: the histogram results side by side (as assign_histogram(flat=True) lays them out), then extras"""

    def __init__(self, host, hist_len):
        self.host, self.pos, self.extra = host, 0, hist_len

    def take(self, n, g):
        o = self.pos
        self.pos += 2 * n + n * g + g
        h = self.host
        return h[o:o + n], h[o + n:o + 2 * n], h[o + 2 * n:o + 2 * n + n * g].reshape(n, g), h[o + 2 * n + n * g:self.pos]

    def more(self, k):
        o = self.extra
        self.extra += k
        return self.host[o:o + k]


def _score_bits(scores):
    return scores.contiguous().view(torch.int32).to(torch.int64)


def _scores_of(bits):
    return bits.astype(np.int32).view(np.float32)


def _sizes(batched_inputs, images):
    isz = [(int(s[0]), int(s[1])) for s in images.image_sizes]
    return isz, [(int(inp.get("height", s[0])), int(inp.get("width", s[1]))) for inp, s in zip(batched_inputs, isz)]


def _resized_targets(masks, objects, isz, osz):
    """one pd_masks_resize_u8 launch -> (part masks bool [G, H, W], object mask bool [H, W]) per image"""
    resized = G.masks_resize([x for m, o, i, s in zip(masks, objects, isz, osz) for x in ((m.bool(), i, s), (o.bool(), i, s))])
    tms = [r[0] for r in resized[0::2]]
    tos = [(r[0][0] if r[0].shape[0] == 1 else r[0].any(0)) for r in resized[1::2]]
    return tms, tos


def _object_label(label, inp):
    """the object class as a Python int: from the mapper's CPU tensor where there is one (no synchronisation), else from the target"""
    try:
        c = inp["instances"].gt_classes
        if torch.is_tensor(c) and not c.is_cuda and c.numel() == 1:
            return int(c)
    except (AttributeError, KeyError, TypeError):
        pass
    return int(label)


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)


def _within_limits(K, Q, gs, keys=1):
    return 1 <= K <= A.MAX_K and 1 <= Q <= A.MAX_Q and all(g <= A.MAX_GT for g in gs) and 1 <= keys <= A.MAX_KEYS


def _gt_instances(tm, labels=None):
    gt = Instances(tuple(tm.shape[-2:]))
    gt.gt_masks, gt.pred_masks = tm, tm
    if labels is not None:
        gt.gt_classes = labels
    return gt


def _classes_batch(what, sel, logits_all, tms, tos, masked, pad_hw, isz, osz, thresholds):
    """the class-aware core of pd_fused and rank_label_fused.  sel: per image (scores fp32 [K], pair_query int64 [K], labels int64 [K],
    keys of the class histogram) -> per image (class map int16 [H, W], scores, classes, best pairs, best ground-truth masks as host arrays)"""
    items = [(low.float(), q.to(torch.int32), scores, to if masked else None, labels.to(torch.int32), pad_hw, i, o)
             for low, (scores, q, labels, _), to, i, o in zip(logits_all, sel, tos, isz, osz)]
    maps = A.pair_assign_resized(items)
    hist = []
    for (arg, obj, _, clsmap), tm, (scores, _, _, n) in zip(maps, tms, sel):
        hist += [(arg, obj, None, scores.shape[0]), (clsmap, obj, tm if tm.shape[0] else None, n)]
    _, flat = A.assign_histogram(hist, flat=True)
    host = _Counts(read_counts(torch.cat([flat] + [x for scores, _, labels, _ in sel for x in (labels.to(torch.int64), _score_bits(scores))])),
                   flat.numel())
    out = []
    for (_, _, _, clsmap), tm, (scores, _, _, n) in zip(maps, tms, sel):
        K = scores.shape[0]
        won = host.take(K, 0)[0]
        _, area_c, inter_c, gt_area = host.take(n, tm.shape[0])
        labels_h, scores_h = host.more(K), _scores_of(host.more(K))
        try:
            out.append((clsmap,) + decide_classes(won, labels_h, scores_h, area_c, inter_c, gt_area, *thresholds))
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
    return out


def pd_fused(model, batched_inputs, targets, images, cls_all, logits_all, vis=False):
    """inference.pd_inference, per-pixel-unique, for a whole batch; None when a kernel limit does not hold"""
    nc, topk, eval_mode = model.num_part_classes, model.test_topk_per_image, model.mode == "eval"
    keys = A.MAX_KEYS if eval_mode else nc                            # the mapped labels' range is the mapping's: checked after the read-back
    if cls_all.shape[-1] - 1 != nc or not _within_limits(topk, logits_all.shape[1], [t["masks"].shape[0] for t in targets], keys):
        return None
    dev = logits_all.device
    pad_hw = tuple(int(s) for s in images.tensor.shape[-2:])
    isz, osz = _sizes(batched_inputs, images)
    tms, tos = _resized_targets([t["masks"] for t in targets], [t["object_mask"] for t in targets], isz, osz)
    sel = []
    for cls, tgt, inp in zip(cls_all, targets, batched_inputs):
        scores, idx = cls.float().softmax(-1)[:, :-1].flatten(0, 1).topk(topk, sorted=False)
        labels = idx % nc
        if eval_mode:
            labels = model.majority_vote_mapping[_object_label(tgt["gt_object_class"], inp)][labels]
        sel.append((scores, torch.div(idx, nc, rounding_mode="floor"), labels, keys))
    decided = _classes_batch("pd_inference", sel, logits_all, tms, tos, model.apply_masking_with_object_mask, pad_hw, isz, osz,
                             (model.min_pseudo_mask_ratio, model.min_pseudo_mask_score, model.fg_score_threshold))
    results = []
    for (clsmap, classes, best, gt_idx), (scores, _, _, _), tm, tgt, inp, (H, W) in zip(decided, sel, tms, targets, batched_inputs, osz):
        if classes.size:
            labels = _to_dev(classes, dev)
            masks = clsmap[None] == labels[:, None, None].to(torch.int16)
            sc, gt_labels = scores[_to_dev(best, dev)], tgt["labels"][_to_dev(gt_idx, dev)]
        else:                                                            # does not contribute to the evaluation
            masks = torch.zeros((1, H, W), dtype=torch.bool, device=dev)
            sc = scores.new_zeros(1)
            labels = gt_labels = torch.full((1,), nc, dtype=torch.long, device=dev)
        r = Instances((H, W))
        r.pred_masks, r.scores, r.pred_classes = masks, sc, (gt_labels if model.use_oracle_classifier else labels)
        if model.mode == "save" and not vis:
            D.save_part_segmentation(model, inp, r)
        gt = _gt_instances(tm, tgt["labels"])
        gt.pred_classes = tgt["labels"]
        results.append({"predictions": r, "gt_instances": gt, "gt_object_label": tgt["gt_object_class"]})
    return results


def _rank_tail(res, tm, tgt, n_rows):
    res["gt_instances"] = _gt_instances(tm, tgt.get("part_labels"))
    res["gt_object_label"] = tgt["object_label"]
    res["gt_label"] = tgt["object_label"].reshape(-1)[:1].repeat(n_rows)
    return res


def rank_label_fused(model, batched_inputs, targets, images, cls_all, logits_all, feats_all, vis=False):
    """inference.rank_inference in the labelling modes ("", "eval", "save"), per-pixel-unique, for a whole batch; None when a kernel limit
    does not hold"""
    topk, eval_mode = model.test_topk_per_image, model.mode == "eval"
    cids = [_object_label(tgt["object_label"], inp) for tgt, inp in zip(targets, batched_inputs)]
    ncs = [model.classifier[c].shape[0] if c in model.classifier else 0 for c in cids]
    if not _within_limits(topk, logits_all.shape[1], [t["masks"].shape[0] for t in targets], max(ncs + [1])):
        return None
    dev = logits_all.device
    pad_hw = tuple(int(s) for s in images.tensor.shape[-2:])
    isz, osz = _sizes(batched_inputs, images)
    tms, tos = _resized_targets([t["masks"] for t in targets], [t["object_mask"] for t in targets], isz, osz)
    sel = []
    for cls, feats, cid, nc in zip(cls_all, feats_all, cids, ncs):
        scores = cls.float().softmax(-1)[:, :1] * D.rank_use_classifier(model, feats, cid).softmax(-1)
        scores, idx = scores.flatten().topk(topk, sorted=False)
        labels = idx % nc
        if eval_mode:
            if len(model.majority_vote_mapping) == 0:
                raise ValueError("Class mapping is not registered.")
            labels = model.majority_vote_mapping[cid][labels]
        sel.append((scores, torch.div(idx, nc, rounding_mode="floor"), labels, A.MAX_KEYS if eval_mode else nc))
    decided = _classes_batch("rank_inference", sel, logits_all, tms, tos, model.apply_masking_with_object_mask, pad_hw, isz, osz,
                             (model.min_pseudo_mask_ratio_2, model.min_pseudo_mask_score_2, model.fg_score_threshold))
    results = []
    for (clsmap, classes, best, _), (scores, _, _, _), tm, tgt, inp, feats, (H, W) in zip(decided, sel, tms, targets, batched_inputs,
                                                                                         feats_all, osz):
        if classes.size:
            labels = _to_dev(classes, dev)
            masks = clsmap[None] == labels[:, None, None].to(torch.int16)
            sc = scores[_to_dev(best, dev)]
        else:                                                            # does not contribute to the evaluation
            masks = torch.zeros((1, H, W), dtype=torch.bool, device=dev)
            sc, labels = scores.new_zeros(1), torch.zeros(1, dtype=torch.long, device=dev)
        r = Instances((H, W))
        r.pred_masks, r.scores, r.pred_classes = masks, sc, labels
        if model.mode == "save" and not vis:
            D.save_generated_part_labels(model, inp, tgt["object_label"], r)
        results.append(_rank_tail({"predictions": r}, tm, tgt, feats.shape[0]))
    return results


def rank_cluster_fused(model, batched_inputs, targets, images, cls_all, logits_all, feats_all):
    """inference.rank_inference in mode "cluster", per-pixel-unique, for a whole batch; None when a kernel limit does not hold.  The
    assignment runs without the object mask (the reference filters on unmasked areas); the object mask is applied after the filters, and
    the IoUs are those of the masked proposals: a second histogram over the same arg map with obj & object mask."""
    topk = model.test_topk_per_image
    if cls_all.shape[-1] != 2 or not _within_limits(topk, logits_all.shape[1], [t["masks"].shape[0] for t in targets]):
        return None                                                      # (more than one object class: the reference indexes queries by a pair index)
    dev = logits_all.device
    pad_hw = tuple(int(s) for s in images.tensor.shape[-2:])
    isz, osz = _sizes(batched_inputs, images)
    tms, tos = _resized_targets([t["masks"] for t in targets], [t["object_mask"] for t in targets], isz, osz)
    sel = [cls.float().softmax(-1)[:, :-1].flatten().topk(topk, sorted=False) for cls in cls_all]
    maps = A.pair_assign_resized([(low.float(), idx.to(torch.int32), scores, None, None, pad_hw, i, o)
                                  for low, (scores, idx), i, o in zip(logits_all, sel, isz, osz)])
    hist = []
    for (arg, obj, _, _), tm, to in zip(maps, tms, tos):
        inside = (obj.bool() & to) if model.apply_masking_with_object_mask else obj
        hist += [(arg, obj, None, topk), (arg, inside, tm if tm.shape[0] else None, topk)]
    _, flat = A.assign_histogram(hist, flat=True)
    host = _Counts(read_counts(torch.cat([flat] + [_score_bits(scores) for scores, _ in sel])), flat.numel())
    results = []
    for i, ((arg, _, _, _), tm, (scores, idx), feats, tgt) in enumerate(zip(maps, tms, sel, feats_all, targets)):
        won, area, _, _ = host.take(topk, 0)
        _, area_in, inter, gt_area = host.take(topk, tm.shape[0])
        keep = decide_queries(won, area, _scores_of(host.more(topk)), model.min_pseudo_mask_ratio_1, model.min_pseudo_mask_score_1)
        fg, _ = match_rows(area_in[keep], inter[keep], gt_area, model.fg_score_threshold)
        rows = _to_dev(keep[fg], dev)
        r = Instances(osz[i])
        r.pred_masks = (arg[None] == rows[:, None, None].to(torch.int16)) & hist[2 * i + 1][1].bool()[None]
        r.scores = scores[rows]
        pf = feats[idx][rows]
        results.append(_rank_tail({"predictions": r, "proposal_features": pf}, tm, tgt, pf.shape[0]))
    return results


def proposal_fused(model, batched_inputs, targets, images, cls_all, logits_all, which):
    """inference.inference (ProposalModel), per-pixel-unique, for the images `which` of a batch - those whose output is resized - in one
    pd_mask_assign_resized launch; -> {image index: (masks, scores, labels, part masks bool [G, H, W])}, None when a kernel limit does
    not hold"""
    topk = model.test_topk_per_image
    if not which or not _within_limits(topk, logits_all.shape[1], [targets[b]["masks"].shape[0] for b in which]):
        return None
    dev = logits_all.device
    pad_hw = tuple(int(s) for s in images.tensor.shape[-2:])
    isz, osz = _sizes(batched_inputs, images)
    isz, osz = [isz[b] for b in which], [osz[b] for b in which]
    tms, tos = _resized_targets([targets[b]["masks"] for b in which], [targets[b]["object_masks"] for b in which], isz, osz)
    sel, items = [], []
    for b, to, i, o in zip(which, tos, isz, osz):
        scores = cls_all[b].float().softmax(-1)[:, :-1].topk(1, dim=1)[0].flatten()
        scores, idx = scores.topk(topk, sorted=False)
        sel.append(scores)
        items.append((logits_all[b][idx].float().contiguous(), scores, to if model.apply_masking_with_object_mask else None, None, pad_hw, i, o))
    maps = A.mask_assign_resized(items)
    _, flat = A.assign_histogram([(arg, obj, tm if tm.shape[0] else None, topk) for (arg, obj, _, _), tm in zip(maps, tms)], flat=True)
    host = _Counts(read_counts(torch.cat([flat] + [_score_bits(s) for s in sel])), flat.numel())
    out = {}
    for b, (arg, obj, _, _), tm, scores in zip(which, maps, tms, sel):
        won, area, inter, gt_area = host.take(topk, tm.shape[0])
        keep = decide_queries(won, area, _scores_of(host.more(topk)), model.minimum_pseudo_mask_ratio, model.minimum_pseudo_mask_score)
        fg, gt_idx = match_rows(area[keep], inter[keep], gt_area, 0.001)
        rows = _to_dev(keep[fg], dev)
        masks = (arg[None] == rows[:, None, None].to(torch.int16)) & obj.bool()[None]
        out[b] = (masks, scores[rows], targets[b]["labels"][_to_dev(gt_idx[fg], dev)], tm)
    return out
