"""numpy restatement of the evaluation counters (include/pd_eval.h) for the evaluator tests: bit planes, intersections, label-map
confusion tables and the greedy cover of the box-proposal recall, all from dense bool masks; plus the readers of tests/golden/eval.pt."""
import math

import numpy as np
import torch

LIMITS = (1, 10, 50, 100, 200)


def thresholds():
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32).numpy()


def unpack(rec):
    """{"bits": numpy.packbits of the flattened mask, "shape"} -> bool tensor"""
    shape = tuple(rec["shape"])
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(rec["bits"].numpy(), count=n).astype(bool).reshape(shape))


def pack_words(masks):
    """bool [n, ...] -> int64 [n, ceil(HW / 64)]: pixel q is bit q % 64 of word q / 64"""
    m = np.asarray(masks)
    m = m.reshape(m.shape[0], int(np.prod(m.shape[1:]))).astype(bool)
    n, hw = m.shape
    words = (hw + 63) // 64
    pad = np.zeros((n, words * 64), dtype=np.uint64)
    pad[:, :hw] = m
    return (pad.reshape(n, words, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64).view(np.int64)


def intersections(pred, rows, gt):
    p = np.asarray(pred).reshape(len(pred), -1).astype(np.int64)
    if rows is not None:
        p = p[np.asarray(rows)]
    return p @ np.asarray(gt).reshape(len(gt), -1).astype(np.int64).T


def recall_counts(images):
    """images: [(pred bool [P, H, W], scores [P], gt bool [G, H, W])] -> hits int64 [5, 10], num_pos int64 [5] (the reference's
    _evaluate_box_proposals, area "all", restated)"""
    thr = thresholds()
    hits = np.zeros((len(LIMITS), len(thr)), dtype=np.int64)
    num_pos = np.zeros(len(LIMITS), dtype=np.int64)
    for pred, scores, gt in images:
        pred, gt = np.asarray(pred), np.asarray(gt)
        if pred.shape[0] == 0 or gt.shape[0] == 0:
            continue
        order = torch.sort(torch.as_tensor(scores), descending=True, stable=True)[1].numpy()
        pf = pred.reshape(len(pred), -1)[order].astype(np.int64)
        gf = gt.reshape(len(gt), -1).astype(np.int64)
        ga = gf.sum(1)
        gf = gf[(ga > 0) & (ga <= 1e10)]
        inter = pf @ gf.T
        union = pf.sum(1)[:, None] + gf.sum(1)[None, :] - inter
        iou = np.where(union > 0, inter / np.maximum(union, 1), 0.0)
        for li, limit in enumerate(LIMITS):
            num_pos[li] += gf.shape[0]
            if gf.shape[0] == 0:
                continue
            ov = iou[:limit].copy()
            rec = np.zeros(gf.shape[0], dtype=np.float32)
            for j in range(min(ov.shape[0], ov.shape[1])):
                col_max, col_arg = ov.max(0), ov.argmax(0)
                gi = int(col_max.argmax())
                bi = int(col_arg[gi])
                rec[j] = ov[bi, gi]
                ov[bi, :] = -1
                ov[:, gi] = -1
            hits[li] += (rec[:, None] >= thr[None, :]).sum(0)
    return hits, num_pos


def label_map(masks, classes, n):
    """class of the last mask covering each pixel, n where none does"""
    masks = np.asarray(masks)
    lab = np.full(masks.shape[1:], n, dtype=np.int64)
    for m, c in zip(masks, np.asarray(classes)):
        lab[m.astype(bool)] = c
    return lab


def confusion(images, n, slots):
    """images: [(pred masks, pred classes, gt masks, gt classes, slot)] -> int64 [slots, n + 1, n + 1]"""
    conf = np.zeros((slots, n + 1, n + 1), dtype=np.int64)
    for pm, pc, gm, gc, slot in images:
        pd, g = label_map(pm, pc, n), label_map(gm, gc, n)
        conf[slot] += np.bincount((n + 1) * pd.reshape(-1) + g.reshape(-1), minlength=(n + 1) ** 2).reshape(n + 1, n + 1)
    return conf


def proposal_images(case):
    return [(unpack(i["pred"]), i["scores"], unpack(i["gt"])) for i in case["images"]]


def miou_images(case):
    return [(unpack(i["pred"]), i["pred_classes"], unpack(i["gt"]), i["gt_classes"], i["object"]) for i in case["images"]]


def gt_num_classes(case):
    return len(case.get("part_classes", case["thing_classes"]))


def assert_same_dict(got, want, rel=0.0):
    """equal keys in the same order, equal values (NaN == NaN), floats within `rel` relative"""
    assert list(got.keys()) == list(want.keys()), (list(got.keys()), list(want.keys()))
    for k in want:
        a, b = got[k], want[k]
        if isinstance(b, dict):
            assert_same_dict(a, b, rel)
        elif isinstance(b, float) and math.isnan(b):
            assert isinstance(a, float) and math.isnan(a), (k, a, b)
        elif rel and isinstance(b, float):
            assert abs(a - b) <= rel * abs(b), (k, a, b)
        else:
            assert a == b, (k, a, b)
