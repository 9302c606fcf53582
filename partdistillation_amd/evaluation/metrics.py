"""Host half of the evaluators: the reference's metric formulas applied to the small integer count tables the device produces
(functions/eval_metrics.py), and the one-all_reduce merge of those tables across ranks.

- proposal_metrics: AR@k of proposal_evaluator.py:_evaluate_box_proposals / _eval_proposals (recall per threshold and its mean in
  float32, as the reference computes them from its float32 overlap vector).
- measure_miou / miou_metrics: miou_evaluator.py:measure_mIOU and the C-* / A-* aggregation of its evaluate(), in float64.
- supervised_miou_metrics: supervised_miou_evaluator.py:evaluate (one table, no object classes).
- majority_voting: miou_matcher.py:majority_voting (first index on ties)."""
import logging

import numpy as np
import torch

from ..functions.eval_metrics import LIMITS

logger = logging.getLogger("partdistillation_amd.evaluation")


def merge_counts(t, distributed):
    """sum a fixed-size count table over the ranks (one all_reduce) when running distributed"""
    import torch.distributed as dist
    if distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


def is_main_process():
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


def proposal_metrics(hits, num_pos, images):
    """hits int [5, 10], num_pos int [5] (limits 1, 10, 50, 100, 200), images int -> the reference's result dict
    {"AR@1": .., "# instances": images, "AR@10": .., ...}"""
    hits = np.asarray(hits, dtype=np.int64).reshape(len(LIMITS), -1)
    num_pos = np.asarray(num_pos, dtype=np.int64).reshape(-1)
    res = {}
    for li, limit in enumerate(LIMITS):
        recalls = torch.zeros(hits.shape[1], dtype=torch.float32)
        for t in range(hits.shape[1]):
            # (gt_overlaps >= t).float().sum() / float(num_pos): an exact float32 count divided as a float32 tensor
            recalls[t] = torch.tensor(float(hits[li, t]), dtype=torch.float32) / float(num_pos[li])
        res["AR@{:d}".format(limit)] = float(recalls.mean().item() * 100)
        res["# instances"] = int(images)
    return res


def measure_miou(conf, class_names, num_classes):
    """one object class's confusion matrix [(n + 1), (n + 1)] (rows: prediction, columns: ground truth, last = background)
    -> the reference's per-class and mean IoU / IoPred / ACC dict (percent).  mIoU sums over the classes with ground-truth pixels and
    divides by the number of classes with ground-truth OR predicted pixels, as the reference does."""
    conf = np.asarray(conf, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.full(num_classes, np.nan, dtype=float)
        iou = np.full(num_classes, np.nan, dtype=float)
        iopred = np.full(num_classes, np.nan, dtype=float)
        tp = conf.diagonal()[:-1].astype(float)
        pos_gt = np.sum(conf[:, :-1], axis=0).astype(float)
        pos_pred = np.sum(conf[:-1, :], axis=1).astype(float)
        weights = pos_gt / np.sum(pos_gt)
        has_gt = pos_gt > 0
        has_any = (pos_gt + pos_pred) > 0
        has_pred = pos_pred > 0
        acc[has_gt] = tp[has_gt] / pos_gt[has_gt]
        iou[has_gt] = tp[has_gt] / (pos_gt + pos_pred - tp)[has_gt]
        iopred[has_pred] = tp[has_pred] / pos_pred[has_pred]
        res = {"mIoU": 100 * (np.sum(iou[has_gt]) / np.sum(has_any)),
               "mIoPred": 100 * (np.sum(iopred[has_pred]) / np.sum(has_pred)),
               "fwIoU": 100 * np.sum(iou[has_gt] * weights[has_gt])}
        for prefix, vals in (("IoU-", iou), ("IoPred-", iopred), ("ACC-", acc)):
            for i, name in enumerate(class_names):
                res[f"{prefix}{name}"] = 100 * vals[i]
        res["mACC"] = 100 * (np.sum(acc[has_gt]) / np.sum(has_gt))
        res["pACC"] = 100 * (np.sum(tp) / np.sum(pos_gt))
    return res


def supervised_miou_metrics(conf, class_names, num_classes):
    """supervised_miou_evaluator.py:evaluate on one confusion matrix [(n + 1), (n + 1)]: mIoU is the mean of the per-class IoUs that
    are not NaN (classes with ground-truth pixels), mACC / mIoPred those of measure_mIOU (the same formulas as measure_miou)"""
    r = measure_miou(conf, class_names, num_classes)
    ious = [v for k, v in r.items() if "IoU-" in k and not np.isnan(v)]
    return {"mIoU": np.mean(ious) if ious else np.nan, "mACC": r["mACC"], "mIoPred": r["mIoPred"]}


def seen_slots(conf):
    """object classes (rows of the dense [S, n + 1, n + 1] table) with any count"""
    conf = np.asarray(conf)
    return [int(k) for k in np.flatnonzero(conf.reshape(conf.shape[0], -1).any(1))]


def miou_metrics(conf, class_names, num_classes):
    """dense confusion tables [S, n + 1, n + 1] -> {"C-mIoU", "A-mIoU", "C-mACC", "A-mACC", "C-mIoPred", "A-mIoPred"}: C-* the mean over
    the object classes seen of their class means, A-* the mean over every (object class, part) value that is not NaN"""
    out = {"C-mIoU": [], "A-mIoU": [], "C-mACC": [], "A-mACC": [], "C-mIoPred": [], "A-mIoPred": []}
    for k in seen_slots(conf):
        r = measure_miou(conf[k], class_names, num_classes)
        for metric, key in (("mIoU", "IoU-"), ("mACC", "ACC-"), ("mIoPred", "IoPred-")):
            out["C-" + metric].append(r[metric])
            out["A-" + metric].extend([v for name, v in r.items() if key in name and not np.isnan(v)])
    with np.errstate(invalid="ignore", divide="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)               # np.mean([]) when nothing was seen: NaN, like the reference
            return {k: np.mean(v) for k, v in out.items()}


def majority_voting(conf, pred_num_classes, gt_num_classes):
    """[(n + 1), (n + 1)] -> int64 [pred_num_classes]: for every predicted class the ground-truth class it overlaps most (first on ties)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(conf)[:pred_num_classes, :gt_num_classes].argmax(axis=1)).astype(np.int64))
