"""The host decisions of the fused evaluation routes (partdistillation_amd/inference_fused.py) are pure functions of integer counts.
Here the maps a kernel would write are formed with torch from random logits built directly at the output size (no interpolation is
involved), the counts with numpy, and the decisions are compared with the dense functions of inference.py run on the CPU: masks, scores,
labels and row order must be EQUAL."""
import types

import numpy as np
import pytest
import torch

H, W, K, Q = 9, 13, 12, 5


def _maps(masks, scores, labels=None):
    """what pd_pair_assign_resized writes for masks = logits[pair_query] * object mask: arg, obj and the class map"""
    arg = (scores[:, None, None] * masks.sigmoid()).argmax(0)
    obj = masks.max(dim=0)[0] > 0.0
    cls = None if labels is None else torch.where(obj, labels[arg], torch.full_like(arg, -1))
    return arg, obj, cls


def _histogram(key, obj, gt, n):
    """pd_assign_histogram with numpy: won, area, inter, gt_area (int64)"""
    k, ob = key.numpy().ravel(), obj.numpy().ravel()
    ok = (k >= 0) & (k < n)
    won = np.bincount(k[ok], minlength=n).astype(np.int64)
    area = np.bincount(k[ok & ob], minlength=n).astype(np.int64)
    g = gt.numpy().reshape(gt.shape[0], key.numel())
    inter = np.stack([np.bincount(k[ok & ob & t], minlength=n) for t in g], axis=1).astype(np.int64) if len(g) else np.zeros((n, 0), np.int64)
    return won, area, inter, g.sum(1).astype(np.int64)


def _case(seed, G, repeated=True):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((Q, H, W), generator=g) * 2
    pq = torch.randint(0, Q, (K,), generator=g)
    if repeated:
        pq[3] = pq[0]                                                     # one query under two pairs (two classes below)
    scores = torch.rand((K,), generator=g) * 0.9 + 0.05
    labels = torch.randint(0, 4, (K,), generator=g)
    if repeated:
        labels[0], labels[3] = 1, 2
    obj_in = torch.rand((H, W), generator=g) > 0.25
    gt = torch.rand((G, H, W), generator=g) < 0.4
    return logits, pq, scores, labels, obj_in, gt


def _dense_classes(view, masks, scores, labels, gt, thr):
    from partdistillation_amd import inference as I
    m, s, l = I._unique_assignment_with_classes(view, masks, scores, labels)
    top1, top1_idx = I.mask_iou(m, gt).topk(1, dim=1)
    fg = (top1 > thr).flatten()
    return m[fg], s[fg], l[fg], top1_idx.flatten()[fg]


def _fused_classes(view, masks, scores, labels, gt, thr, n):
    from partdistillation_amd import inference_fused as FU
    arg, obj, cls = _maps(masks, scores, labels)
    won = _histogram(arg, obj, gt[:0], K)[0]
    _, area_c, inter_c, gt_area = _histogram(cls, obj, gt, n)
    classes, best, gt_idx = FU.decide_classes(won, labels.numpy(), scores.numpy(), area_c, inter_c, gt_area, view.min_pseudo_mask_ratio,
                                              view.min_pseudo_mask_score, thr)
    c = torch.from_numpy(classes)
    return cls[None] == c[:, None, None], scores[torch.from_numpy(best)], c, torch.from_numpy(gt_idx)


def _view(ratio, score):
    return types.SimpleNamespace(use_unique_per_pixel_label=True, min_pseudo_mask_ratio=ratio, min_pseudo_mask_score=score)


def _assert_same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b), (a, b)


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("ratio,score", [(0.02, -1.0), (0.1, 0.3), (2.0, 2.0)])      # (2.0, 2.0): both filters would remove everything -> skipped
@pytest.mark.parametrize("mapping", [None, [2, 0, 0, 1]])                             # two clusters mapped to one class ("eval")
def test_class_merge_filters_and_match_equal_the_dense_route(G, ratio, score, mapping):
    logits, pq, scores, labels, obj_in, gt = _case(100 + G, G)
    if mapping is not None:
        labels = torch.tensor(mapping)[labels]
    masks = logits[pq] * obj_in
    view = _view(ratio, score)
    want = _dense_classes(view, masks, scores, labels, gt, 0.1)
    got = _fused_classes(view, masks, scores, labels, gt, 0.1, 1024 if mapping is not None else 4)
    assert want[0].shape[0] >= 1
    if (ratio, score) == (2.0, 2.0):                                      # nothing was filtered: every class of a winning pair is there
        assert want[0].shape[0] == _dense_classes(_view(-1.0, -1.0), masks, scores, labels, gt, 0.1)[0].shape[0]
    _assert_same(got, want)


def test_shared_query_ties_go_to_the_first_pair():
    """two pairs of one query with EQUAL scores tie on every pixel: the arg-max takes the first, the second wins nothing and its class
    appears only through other pairs"""
    logits, pq, scores, labels, obj_in, gt = _case(7, 2)
    scores[3] = scores[0]
    labels[3] = 3
    labels[labels == 3] = 0
    labels[3] = 3                                                         # class 3 is carried by pair 3 alone
    masks = logits[pq] * obj_in
    got = _fused_classes(_view(-1.0, -1.0), masks, scores, labels, gt, -1.0, 4)
    want = _dense_classes(_view(-1.0, -1.0), masks, scores, labels, gt, -1.0)
    _assert_same(got, want)
    assert 3 not in got[2].tolist()


def test_no_foreground_match_and_no_ground_truth_give_no_rows():
    from partdistillation_amd import inference_fused as FU
    logits, pq, scores, labels, obj_in, gt = _case(9, 3)
    masks = logits[pq] * obj_in
    got = _fused_classes(_view(0.02, -1.0), masks, scores, labels, gt, 1.5, 4)               # no IoU exceeds 1.5: the callers' empty fallback
    want = _dense_classes(_view(0.02, -1.0), masks, scores, labels, gt, 1.5)
    assert got[0].shape[0] == 0
    _assert_same(got, want)
    none = _fused_classes(_view(0.02, -1.0), masks, scores, labels, gt[:0], -1.0, 4)          # G = 0 (the dense route cannot take it)
    assert none[0].shape[0] == 0 and none[3].shape[0] == 0
    fg, idx = FU.match_rows(np.array([3, 4]), np.zeros((2, 0), np.int64), np.zeros((0,), np.int64), -1.0)
    assert not fg.any() and idx.shape == (2,)
    # the stage before the match with G = 0: a single all-true mask and a threshold below every IoU keep all rows
    full = torch.ones((1, H, W), dtype=torch.bool)
    _assert_same(_fused_classes(_view(0.1, 0.3), masks, scores, labels, full, -1.0, 4)[:3],
                 _dense_classes(_view(0.1, 0.3), masks, scores, labels, full, -1.0)[:3])


def test_label_outside_the_histogram_raises():
    from partdistillation_amd import inference_fused as FU
    from partdistillation_amd.functions import mask_assign as A
    logits, pq, scores, labels, obj_in, gt = _case(11, 1)
    labels[5] = A.MAX_KEYS
    with pytest.raises(ValueError, match=f"{A.MAX_KEYS}.*PD_ASSIGN_MAX_KEYS"):
        _fused_classes(_view(0.02, -1.0), logits[pq] * obj_in, scores, labels, gt, 0.1, A.MAX_KEYS)
    labels[5] = -1
    with pytest.raises(ValueError, match="-1 lies outside"):
        _fused_classes(_view(0.02, -1.0), logits[pq] * obj_in, scores, labels, gt, 0.1, A.MAX_KEYS)


def _rank_model(ratio, score, thr=0.1, masking=True):
    return types.SimpleNamespace(use_unique_per_pixel_label_during_clustering=True, min_pseudo_mask_ratio_1=ratio, min_pseudo_mask_score_1=score,
                                 fg_score_threshold=thr, apply_masking_with_object_mask=masking, wandb_vis_topk=K, test_topk_per_image=K)


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("ratio,score,masking", [(0.02, -1.0, True), (0.08, 0.4, True), (2.0, 2.0, True), (0.02, 0.2, False)])
def test_cluster_rows_equal_the_dense_route(G, ratio, score, masking):
    """mode "cluster": the assignment and the filters see the UNMASKED logits, the object mask comes after them, the IoUs are the masked
    proposals'"""
    from partdistillation_amd import inference as I
    from partdistillation_amd import inference_fused as FU
    g = torch.Generator().manual_seed(40 + G)
    logits = torch.randn((K + 3, H, W), generator=g) * 2
    cls_logits = torch.randn((K + 3, 2), generator=g)
    feats = torch.randn((K + 3, 6), generator=g)
    to = (torch.rand((1, H, W), generator=g) > 0.3)
    gt = torch.rand((G, H, W), generator=g) < 0.4
    model = _rank_model(ratio, score, masking=masking)
    m, s, f = I.rank_instance_inference_with_proposal_feats(model, feats, cls_logits, logits, to)
    want = I._rank_match_gt(model, m, s, f, gt)
    scores, idx = cls_logits.float().softmax(-1)[:, :-1].flatten().topk(K, sorted=False)
    arg, obj, _ = _maps(logits[idx], scores)
    inside = obj & to[0] if masking else obj
    won, area, _, _ = _histogram(arg, obj, gt[:0], K)
    _, area_in, inter, gt_area = _histogram(arg, inside, gt, K)
    keep = FU.decide_queries(won, area, scores.numpy(), ratio, score)
    fg, _ = FU.match_rows(area_in[keep], inter[keep], gt_area, model.fg_score_threshold)
    rows = torch.from_numpy(keep[fg])
    got = ((arg[None] == rows[:, None, None]) & inside[None], scores[rows], feats[idx][rows])
    assert want[0].shape[0] >= 1
    _assert_same(got, (want[0].bool(), want[1], want[2]))


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("ratio,score", [(0.02, -1.0), (0.08, 0.6), (2.0, 2.0)])
def test_proposal_rows_equal_instance_inference_dense(G, ratio, score):
    from partdistillation_amd import inference as I
    from partdistillation_amd import inference_fused as FU
    g = torch.Generator().manual_seed(60 + G)
    logits = torch.randn((K + 3, H, W), generator=g) * 2
    cls_logits = torch.randn((K + 3, 2), generator=g)
    to = (torch.rand((1, H, W), generator=g) > 0.3)
    gt = torch.rand((G, H, W), generator=g) < 0.4
    gt_labels = torch.arange(G) + 5
    model = types.SimpleNamespace(use_unique_per_pixel_label=True, apply_masking_with_object_mask=True, minimum_pseudo_mask_ratio=ratio,
                                  minimum_pseudo_mask_score=score)
    want = I.instance_inference_dense(model, cls_logits, logits, gt, to, gt_labels, K)
    scores = cls_logits.float().softmax(-1)[:, :-1].topk(1, dim=1)[0].flatten()
    scores, idx = scores.topk(K, sorted=False)
    arg, obj, _ = _maps(logits[idx] * to, scores)
    won, area, inter, gt_area = _histogram(arg, obj, gt, K)
    keep = FU.decide_queries(won, area, scores.numpy(), ratio, score)
    fg, gt_idx = FU.match_rows(area[keep], inter[keep], gt_area, 0.001)
    rows = torch.from_numpy(keep[fg])
    got = ((arg[None] == rows[:, None, None]) & obj[None], scores[rows], gt_labels[torch.from_numpy(gt_idx[fg])])
    assert want[0].shape[0] >= 1
    _assert_same(got, want)


def test_rank_match_keeps_the_predicted_labels():
    """the labelling modes: _rank_match_gt after the class merge, the *_2 thresholds"""
    from partdistillation_amd import inference as I
    logits, pq, scores, labels, obj_in, gt = _case(21, 3)
    masks = logits[pq] * obj_in
    view = _view(0.05, 0.2)
    model = types.SimpleNamespace(fg_score_threshold=0.15)
    want = I._rank_match_gt(model, *I._unique_assignment_with_classes(view, masks, scores, labels), gt)
    got = _fused_classes(view, masks, scores, labels, gt, 0.15, 4)
    assert want[0].shape[0] >= 1
    _assert_same(got[:3], want)


def test_switch_and_cpu_tensors_take_the_dense_route(monkeypatch):
    from partdistillation_amd import inference_fused as FU
    monkeypatch.delenv("PD_FUSED_INFERENCE", raising=False)
    assert FU.enabled()
    monkeypatch.setenv("PD_FUSED_INFERENCE", "0")
    assert not FU.enabled()
    assert not FU._within_limits(257, 100, [3]) and not FU._within_limits(200, 1025, [3]) and not FU._within_limits(200, 100, [65])
    assert not FU._within_limits(200, 100, [3], 1025) and FU._within_limits(256, 1024, [64, 0], 1024)
