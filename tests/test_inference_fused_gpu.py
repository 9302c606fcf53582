"""The fused evaluation routes of inference.py (partdistillation_amd/inference_fused.py) against the dense routes (PD_FUSED_INFERENCE=0) on
the inference inputs of tests/golden/common.py: a batch of two, the second image with an output resize.  The kernels interpolate in
their own order of operations, so a mask may differ from the dense one in a few pixels (the bound of test_propgen_gpu.py: 2e-3 of the
pixels); classes and scores are equal, rows come in the dense route's order.  Before comparing, the dense run itself must show that
every decision keeps a margin of 0.01 (area ratios against the ratio threshold, best IoUs against the foreground threshold): a few
pixels then cannot change a set.  The host logic is exact: fed with the kernel's own maps, a dense torch restatement gives the fused
result bit for bit."""
import os
import types

import pytest
import torch

import common as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 0.01
# Seed of make_infer_inputs.  The goldens' own seed (5200) leaves a best IoU 0.005 from its threshold in two branches; of the seeds
# 5200..5215, run through the dense route on the CPU (run_dense_with_margins(branch, ..., dev="cpu")), 5206 is the first with which every
# branch keeps more than MARGIN on both kinds of decision (smallest distances: area ratio 0.012, best IoU 0.030).
SEED = 5206

# branch -> (entry point, mode); every labelling mode and the clustering mode of PartRankingModel, the three modes of PartDistillationModel
BRANCHES = {"proposal": ("inference", None), "pd_raw": ("pd_inference", ""), "pd_eval": ("pd_inference", "eval"), "pd_save": ("pd_inference", "save"),
            "rank_raw": ("rank_inference", ""), "rank_eval": ("rank_inference", "eval"), "rank_save": ("rank_inference", "save"),
            "rank_cluster": ("rank_inference", "cluster")}


def _setup(branch, dev=DEV, root=None, seed=SEED):
    """-> (entry point, model, batched inputs, targets, images, outputs) as the golden tests of the branch build them"""
    from partdistillation_amd import inference as I
    from partdistillation_amd.compat import BitMasks, ImageList, Instances
    fn, mode = BRANCHES[branch]
    outputs, inputs = C.make_infer_inputs(seed=seed)
    topk, nc = C.INFER["topk"], C.INFER_PD_CLASSES
    common = dict(device=torch.device(dev), apply_masking_with_object_mask=True, mode=mode, root_save_path=root)
    if fn == "inference":
        model = types.SimpleNamespace(test_topk_per_image=topk, wandb_vis_topk=topk, use_unique_per_pixel_label=True, minimum_pseudo_mask_ratio=0.02,
                                      minimum_pseudo_mask_score=-1.0, **common)
        outputs = {k: v.to(dev) for k, v in outputs.items()}
        prepare = I.prepare_gt_targets
    elif fn == "pd_inference":
        model = types.SimpleNamespace(test_topk_per_image=topk * 2, wandb_vis_topk=topk * 2, use_unique_per_pixel_label=True, min_pseudo_mask_ratio=0.02,
                                      min_pseudo_mask_score=-1.0, num_part_classes=nc, fg_score_threshold=0.1, use_oracle_classifier=False,
                                      majority_vote_mapping={3: torch.tensor(C.INFER_PD_MAPPING[0], device=dev),
                                                             4: torch.tensor(C.INFER_PD_MAPPING[1], device=dev)}, **common)
        outputs = {"pred_masks": outputs["pred_masks"].to(dev), "pred_logits": (C.seeded((len(inputs), C.INFER["Q"], nc + 1), seed + 100) * 2).to(dev)}
        prepare = I.prepare_pd_gt_targets
    else:
        k = topk if mode == "cluster" else topk * 2
        feats, _, _ = C.make_rank_features()
        model = types.SimpleNamespace(test_topk_per_image=k, wandb_vis_topk=k, classifier_metric="l2", num_queries=C.INFER["Q"], fg_score_threshold=0.1,
                                      use_unique_per_pixel_label_during_clustering=True, use_unique_per_pixel_label_during_labeling=True,
                                      min_pseudo_mask_ratio_1=0.02, min_pseudo_mask_ratio_2=0.02, min_pseudo_mask_score_1=0.05,
                                      min_pseudo_mask_score_2=0.0, proposal_key="decoder_output", proposal_features_norm=True,
                                      classifier={c: v.to(dev) for c, v in C.rank_centroids().items()},
                                      majority_vote_mapping={3: torch.tensor(C.RANK_MAPPING[0], device=dev), 4: torch.tensor(C.RANK_MAPPING[1], device=dev)},
                                      **common)
        outputs = {"pred_masks": outputs["pred_masks"].to(dev), "pred_logits": outputs["pred_logits"].to(dev), "decoder_output": feats.to(dev)}
        prepare = I.rank_prepare_targets
    batched = []
    for b, i in enumerate(inputs):
        parts, objs = Instances(tuple(i["image"].shape[-2:])), Instances(tuple(i["image"].shape[-2:]))
        parts.gt_masks, parts.gt_classes = BitMasks(i["part_masks"]), i["part_labels"]
        objs.gt_masks, objs.gt_classes = BitMasks(i["object_mask"]), torch.tensor([3 + b])
        batched.append({"image": i["image"], "part_instances": parts, "instances": objs, "height": i["height"], "width": i["width"],
                        "file_name": f"img{b}.jpg", "image_id": f"id{b}", "class_code": f"n{b}"})
    images = ImageList.from_tensors([i["image"].to(dev) for i in inputs], C.INFER["size_div"])
    return getattr(I, fn), model, batched, prepare(model, batched, images), images, outputs


def _thresholds(model, branch):
    """(ratio threshold, foreground threshold) of the branch"""
    if branch == "proposal":
        return model.minimum_pseudo_mask_ratio, 0.001
    if branch.startswith("pd"):
        return model.min_pseudo_mask_ratio, model.fg_score_threshold
    return (model.min_pseudo_mask_ratio_1 if branch == "rank_cluster" else model.min_pseudo_mask_ratio_2), model.fg_score_threshold


def run_dense_with_margins(branch, monkeypatch, dev=DEV, root=None, seed=SEED):
    """the dense route, recording every area ratio that meets the ratio filter and every best IoU that meets the foreground threshold
    -> (results, smallest distance of a ratio from its threshold, smallest distance of a best IoU from its threshold)"""
    from partdistillation_amd import inference as I
    fn, model, batched, targets, images, outputs = _setup(branch, dev, root, seed)
    ratio_thr, fg_thr = _thresholds(model, branch)
    ratios, ious = [], []
    real_filter, real_iou = I._filter, I.mask_iou

    def rec_filter(masks_area, obj_area, scores, min_ratio, min_score):
        assert min_ratio == ratio_thr
        ratios.append((masks_area.double() / obj_area.double()).cpu())
        return real_filter(masks_area, obj_area, scores, min_ratio, min_score)

    def rec_iou(pr, gt):
        iou = real_iou(pr, gt)
        if iou.shape[0]:
            ious.append(iou.max(dim=1)[0].cpu())
        return iou

    with monkeypatch.context() as m:
        m.setenv("PD_FUSED_INFERENCE", "0")
        m.setattr(I, "_filter", rec_filter)
        m.setattr(I, "mask_iou", rec_iou)
        res = fn(model, batched, targets, images, outputs)
    assert len(ratios) == 2 and len(ious) == 2                                     # both images reached both decisions
    return res, float((torch.cat(ratios) - ratio_thr).abs().min()), float((torch.cat(ious) - fg_thr).abs().min())


def _fields(r):
    """every tensor a result holds, by name"""
    out = {}
    for key, v in r.items():
        if torch.is_tensor(v):
            out[key] = v
        else:
            for name, t in v.get_fields().items():
                out[f"{key}.{name}"] = t.tensor if hasattr(t, "tensor") else t
    return out


def _compare(fused, dense):
    assert len(fused) == len(dense) == 2
    for rf, rd in zip(fused, dense):
        ff, fd = _fields(rf), _fields(rd)
        assert sorted(ff) == sorted(fd) and sorted(rf) == sorted(rd)
        assert all(tuple(rf[k].image_size) == tuple(rd[k].image_size) for k in rf if not torch.is_tensor(rf[k]))
        for name in ff:
            a, b = ff[name], fd[name]
            assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
            if name in ("predictions.pred_masks", "proposals.pred_masks"):
                assert a.shape[0] >= 1
                diff = (a != b).float().mean().item()
                assert diff < 2e-3, (name, diff)
            else:                                                                 # classes, scores, features, ground truth: equal
                assert torch.equal(a, b), (name, a, b)


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_fused_route_equals_the_dense_route(branch, monkeypatch, tmp_path):
    dense, ratio_margin, iou_margin = run_dense_with_margins(branch, monkeypatch, root=str(tmp_path / "dense"))
    print(f"{branch}: smallest distance of an area ratio from its threshold {ratio_margin:.4f}, of a best IoU {iou_margin:.4f}")
    assert ratio_margin >= MARGIN and iou_margin >= MARGIN, (ratio_margin, iou_margin)
    fn, model, batched, targets, images, outputs = _setup(branch, root=str(tmp_path / "fused"))
    monkeypatch.delenv("PD_FUSED_INFERENCE", raising=False)
    fused = fn(model, batched, targets, images, outputs)
    assert any(tuple(r[k].image_size) != tuple(s) for r, s in zip(fused, images.image_sizes) for k in r if k in ("predictions", "proposals"))
    _compare(fused, dense)


# ------------------------------------------------------------------------------------------------- exactness of the host logic
def _restate_classes(arg, obj, cls, scores, labels, tm, ratio, min_score, fg_thr):
    """inference._unique_assignment_with_classes and the match on the kernel's own maps, with dense [P, H, W] masks"""
    from partdistillation_amd import inference as I
    argl, objb = arg.long(), obj.bool()
    ids = argl.unique()
    new_labels = labels[ids].unique()
    masks = cls.long()[None] == new_labels[:, None, None]
    per_pair = torch.where(labels[None, ids] == new_labels[:, None], scores[None, ids], scores.new_full((), -1.0))
    new_scores = per_pair.max(dim=1)[0]
    keep = I._filter(masks.flatten(1).sum(1), objb.sum(), new_scores, ratio, min_score)
    masks, new_scores, new_labels = masks[keep], new_scores[keep], new_labels[keep]
    top1, top1_idx = I.mask_iou(masks, tm).topk(1, dim=1)
    fg = (top1 > fg_thr).flatten()
    return masks[fg], new_scores[fg], new_labels[fg]


def _restate_queries(arg, obj, inside, scores, tm, ratio, min_score, fg_thr):
    from partdistillation_amd import inference as I
    argl, objb = arg.long(), obj.bool()
    ids = argl.unique()
    masks = (argl[None] == ids[:, None, None]) & objb[None]
    keep = I._filter(masks.flatten(1).sum(1), objb.sum(), scores[ids], ratio, min_score)
    masks, ids = masks[keep] & inside.bool()[None], ids[keep]
    top1, top1_idx = I.mask_iou(masks, tm).topk(1, dim=1)
    fg = (top1 > fg_thr).flatten()
    return masks[fg], scores[ids[fg]], top1_idx.flatten()[fg]


@pytest.mark.parametrize("branch", ["proposal", "pd_eval", "rank_raw", "rank_cluster"])
def test_host_logic_is_exact_on_the_kernels_own_maps(branch, monkeypatch):
    from partdistillation_amd import inference_fused as FU
    fn, model, batched, targets, images, outputs = _setup(branch)
    seen = {}
    for name in ("pair_assign_resized", "mask_assign_resized"):
        def spy(items, real=getattr(FU.A, name), name=name):
            seen["items"], seen["maps"], seen["kernel"] = items, real(items), name
            return seen["maps"]
        monkeypatch.setattr(FU.A, name, spy)
    real_hist = FU.A.assign_histogram

    def spy_hist(items, flat=False):
        seen["hist"] = items
        return real_hist(items, flat=flat)
    monkeypatch.setattr(FU.A, "assign_histogram", spy_hist)
    res = fn(model, batched, targets, images, outputs)
    ratio, fg_thr = _thresholds(model, branch)
    which = [1] if branch == "proposal" else [0, 1]                               # ProposalModel: only the resized image goes this way
    assert seen["kernel"] == ("mask_assign_resized" if branch == "proposal" else "pair_assign_resized") and len(seen["maps"]) == len(which)
    for n, b in enumerate(which):
        arg, obj, _, cls = seen["maps"][n]
        p = res[b]["proposals" if branch == "proposal" else "predictions"]
        tm = res[b]["gt_masks" if branch == "proposal" else "gt_instances"].gt_masks
        if branch == "proposal":
            scores = seen["items"][n][1]
            masks, sc, gt_idx = _restate_queries(arg, obj, obj, scores, tm, ratio, model.minimum_pseudo_mask_score, fg_thr)
            want = (masks, sc, targets[b]["labels"][gt_idx])
        elif branch == "rank_cluster":
            scores, inside = seen["items"][n][2], seen["hist"][2 * n + 1][1]
            want = _restate_queries(arg, obj, inside, scores, tm, ratio, model.min_pseudo_mask_score_1, fg_thr)[:2]
        else:
            scores, labels = seen["items"][n][2], seen["items"][n][4].long()
            min_score = model.min_pseudo_mask_score if branch.startswith("pd") else model.min_pseudo_mask_score_2
            want = _restate_classes(arg, obj, cls, scores, labels, tm, ratio, min_score, fg_thr)
        got = (p.pred_masks, p.scores) + ((p.pred_classes,) if branch != "rank_cluster" else ())
        assert want[0].shape[0] >= 1
        for a, w in zip(got, want):
            assert a.shape == w.shape and torch.equal(a, w)


@pytest.mark.parametrize("branch", ["proposal", "pd_raw", "rank_eval", "rank_cluster"])
def test_one_read_back_per_batch(branch, monkeypatch):
    from partdistillation_amd import inference_fused as FU
    fn, model, batched, targets, images, outputs = _setup(branch)
    calls, real = [], FU.read_counts
    monkeypatch.setattr(FU, "read_counts", lambda t: calls.append(t.numel()) or real(t))
    fn(model, batched, targets, images, outputs)
    assert len(calls) == 1, calls


@pytest.mark.parametrize("branch", ["pd_save", "rank_save"])
def test_saved_labels_decode_to_the_returned_masks(branch, tmp_path):
    from partdistillation_amd.utils import rle
    fn, model, batched, targets, images, outputs = _setup(branch, root=str(tmp_path))
    res = fn(model, batched, targets, images, outputs)
    for r, inp in zip(res, batched):
        p = r["predictions"]
        saved = torch.load(os.path.join(str(tmp_path), inp["class_code"], inp["image_id"]), weights_only=False)
        masks = p.pred_masks.cpu()
        n, H, W = masks.shape
        assert (saved["height"], saved["width"]) == (H, W) == (inp["height"], inp["width"]) and len(saved["part_masks"]) == n >= 1
        for m, e in zip(masks, saved["part_masks"]):
            assert torch.equal(torch.from_numpy(rle.decode(e["segmentation"])), m)
        areas = masks.flatten(1).sum(1)
        assert torch.equal(saved["part_labels"], p.pred_classes.cpu()) and torch.equal(torch.from_numpy(saved["part_scores"]), p.scores.cpu())
        assert saved["object_ratio"] == int(areas.sum()) / (H * W)
        if branch == "pd_save":
            assert torch.equal(saved["part_area_ratios"], areas / int(areas.sum()))
        else:
            assert torch.equal(saved["part_ratios"], areas / (H * W)) and saved["object_class_label"] == int(r["gt_object_label"])


def test_over_limit_sizes_take_the_dense_route(monkeypatch):
    """more pairs than PD_ASSIGN_MAX_K: no kernel is launched, the dense route answers"""
    from partdistillation_amd import inference_fused as FU
    fn, model, batched, targets, images, outputs = _setup("pd_raw")
    monkeypatch.setattr(FU.A, "MAX_K", 8)
    monkeypatch.setattr(FU.A, "pair_assign_resized", lambda items: pytest.fail("the fused route ran"))
    over = fn(model, batched, targets, images, outputs)
    monkeypatch.setenv("PD_FUSED_INFERENCE", "0")
    dense = fn(model, batched, targets, images, outputs)
    for a, b in zip(over, dense):
        assert torch.equal(a["predictions"].pred_masks, b["predictions"].pred_masks)


def test_pd_inference_peak_memory_stays_below_one_dense_stack(monkeypatch):
    """Q = 100, K = 200 pairs, logits 128^2, output 512^2: the fused route's peak growth stays below K * H * W * 4 bytes, one dense fp32
    stack; the dense route builds several"""
    from partdistillation_amd import inference as I
    from partdistillation_amd.compat import BitMasks, ImageList, Instances
    Q, K, nc, low, S = 100, 200, 8, 128, 512
    g = torch.Generator().manual_seed(1)
    base = torch.nn.functional.interpolate(torch.randn((1, Q, 6, 6), generator=g) * 3, size=(low, low), mode="bilinear", align_corners=False)
    outputs = {"pred_masks": (base - 0.8).to(DEV), "pred_logits": (torch.randn((1, Q, nc + 1), generator=g) * 2).to(DEV)}
    ys, xs = torch.meshgrid(torch.arange(S) / S, torch.arange(S) / S, indexing="ij")
    inside = ((ys - 0.5) ** 2 + (xs - 0.5) ** 2) < 0.16
    parts = torch.stack([inside & (xs < 0.4), inside & (xs >= 0.4) & (ys < 0.5), inside & (xs >= 0.4) & (ys >= 0.5)])
    model = types.SimpleNamespace(device=torch.device(DEV), test_topk_per_image=K, wandb_vis_topk=K, use_unique_per_pixel_label=True,
                                  min_pseudo_mask_ratio=0.0, min_pseudo_mask_score=-1.0, num_part_classes=nc, mode="", fg_score_threshold=0.01,
                                  use_oracle_classifier=False, apply_masking_with_object_mask=True, majority_vote_mapping={})
    pi, oi = Instances((S, S)), Instances((S, S))
    pi.gt_masks, pi.gt_classes = BitMasks(parts), torch.tensor([0, 1, 2])
    oi.gt_masks, oi.gt_classes = BitMasks(inside[None]), torch.tensor([3])
    batched = [{"image": torch.zeros((3, S, S)), "part_instances": pi, "instances": oi}]
    images = ImageList.from_tensors([torch.zeros((3, S, S), device=DEV)], 32)
    targets = I.prepare_pd_gt_targets(model, batched, images)
    bound = K * S * S * 4

    def peak():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = I.pd_inference(model, batched, targets, images, outputs)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, res

    peak()                                                                        # (library handles, the pinned ring)
    monkeypatch.delenv("PD_FUSED_INFERENCE", raising=False)
    fused, res = peak()
    monkeypatch.setenv("PD_FUSED_INFERENCE", "0")
    dense, _ = peak()
    print(f"peak growth: fused {fused / 2 ** 20:.1f} MiB, dense {dense / 2 ** 20:.1f} MiB, one dense stack {bound / 2 ** 20:.1f} MiB")
    assert res[0]["predictions"].pred_masks.shape[0] >= 1 and res[0]["predictions"].pred_masks.any()
    assert fused < bound < dense, (fused, bound, dense)
