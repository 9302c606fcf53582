"""Seeded inputs of the SupervisedModel goldens (make_golden_supervised.py) and of the tests that replay them: decoder outputs at low
resolution and per-image ground truth, for output sizes equal to, larger and smaller than the network size, plus one image whose
ground-truth parts lie outside the object (nothing matches).  Own text: nothing here comes from the reference."""
import torch
import torch.nn.functional as F

from common import seeded

# (H, W) the network sees, (out_h, out_w) of the data mapper, kind
SUP = dict(Q=12, low=32, size_div=32, num_classes=8, topk={"agnostic": 8, "classes": 10}, label_classes=3,
           images=[(96, 128, 96, 128, "same"), (128, 112, 171, 150, "up"), (96, 128, 60, 80, "down"), (128, 128, 100, 90, "nomatch")])
PIXEL_MEAN, PIXEL_STD = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]
# tag -> (class_agnostic_learning, use_unique_per_pixel_label)
CONFIGS = {"agnostic_unique": (True, True), "agnostic_plain": (True, False), "classes_unique": (False, True), "classes_plain": (False, False)}


def make_supervised_inputs(cfg=SUP, seed=8128):
    """-> ({"agnostic": decoder outputs with [B, Q, 2] class logits, "classes": with [B, Q, num_classes + 1]}, per-image inputs).
    The mask logits [B, Q, low, low] are smooth blobs (one per query) plus a little noise; the parts are the Voronoi cells of 3 seeded
    centres inside an ellipse (the object), labelled with distinct classes out of the first `label_classes` (so that every
    ground-truth class collects several parts: the evaluator test's tolerance divides by the smallest class area); the `nomatch` image has its parts in a corner strip that
    the object does not touch."""
    B, Q, low = len(cfg["images"]), cfg["Q"], cfg["low"]
    base = F.interpolate(seeded((B, Q, 5, 5), seed + 1) * 3, size=(low, low), mode="bilinear", align_corners=False)
    masks = base + 0.3 * seeded((B, Q, low, low), seed + 2) - 0.8
    outputs = {"agnostic": {"pred_logits": seeded((B, Q, 2), seed) * 2, "pred_masks": masks},
               "classes": {"pred_logits": seeded((B, Q, cfg["num_classes"] + 1), seed + 3) * 2, "pred_masks": masks}}
    inputs = []
    for b, (H, W, oh, ow, kind) in enumerate(cfg["images"]):
        ys, xs = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
        inside = ((ys - 0.5) ** 2 / 0.17 + (xs - 0.5) ** 2 / 0.12) < 1.0
        g = torch.Generator().manual_seed(seed + 30 + b)
        centers = torch.rand((3, 2), generator=g) * 0.5 + 0.25
        lab = torch.stack([(ys - c[0]) ** 2 + (xs - c[1]) ** 2 for c in centers]).argmin(0)
        if kind == "nomatch":
            inside = ((ys - 0.6) ** 2 / 0.1 + (xs - 0.6) ** 2 / 0.1) < 1.0
            parts = torch.stack([(ys < 0.12) & (xs < 0.12 * (k + 1)) & (xs >= 0.12 * k) for k in range(3)])
            assert not bool((parts & inside).any()) and bool(parts.flatten(1).any(1).all())
        else:
            parts = torch.stack([(lab == k) & inside for k in range(3)])
        inputs.append({"image": (seeded((3, H, W), seed + 40 + b) * 50 + 100).clamp(0, 255), "part_masks": parts,
                       "part_labels": torch.randperm(cfg["label_classes"], generator=g)[:3], "object_mask": inside[None], "height": oh, "width": ow})
    return outputs, inputs


def batched_inputs(inputs, Instances, BitMasks, device="cpu"):
    """the model's input dicts (part_instances: part masks + labels, instances: the object mask)"""
    out = []
    for i in inputs:
        H, W = i["part_masks"].shape[-2:]
        parts, obj = Instances((H, W)), Instances((H, W))
        parts.gt_masks, parts.gt_classes = BitMasks(i["part_masks"].to(device)), i["part_labels"].to(device)
        obj.gt_masks = BitMasks(i["object_mask"].to(device))
        out.append({"image": i["image"].to(device), "height": i["height"], "width": i["width"], "part_instances": parts, "instances": obj})
    return out
