"""Inputs of the pixel-grouping evaluation golden (tests/golden/pixel_grouping.pt), shared by make_golden_pixel_grouping.py (build
container, runs the reference) and the tests (never touch the reference): synthetic backbone features in the style of
common.make_propgen_inputs, one elliptical object per image, 2-3 ground-truth part masks cut from it, image / output sizes."""
import numpy as np
import torch
import torch.nn.functional as F

from common import seeded

# (H, W, out_h, out_w, object): identity; crop + down-scale; up-scale; an object of <= K pixels at feature resolution; no object
PIXGROUP = dict(C3=16, C4=24, K=4, size_div=32,
                images=[(128, 128, 128, 128, "ellipse"), (112, 128, 96, 110, "ellipse"), (96, 128, 150, 200, "ellipse"),
                        (128, 128, 100, 90, "tiny"), (112, 96, 112, 96, "empty")])
CONFIGS = (("dot_0", "dot", False), ("l2_1", "l2", True))
PIXEL_MEAN, PIXEL_STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def padded_size(cfg=PIXGROUP):
    d = cfg["size_div"]
    Hp, Wp = max(i[0] for i in cfg["images"]), max(i[1] for i in cfg["images"])
    return (Hp + d - 1) // d * d, (Wp + d - 1) // d * d


def make_pixel_grouping_inputs(cfg=PIXGROUP, seed=6147):
    """-> (features {"res3": [B, C3, Hp/8, Wp/8], "res4": [B, C4, Hp/16, Wp/16]}, [per image: image, object mask bool [1, H, W], part masks
    bool [G, H, W], part labels, height, width])"""
    Hp, Wp = padded_size(cfg)
    B = len(cfg["images"])
    feats = {}
    for key, ch, stride, s0 in (("res3", cfg["C3"], 8, seed), ("res4", cfg["C4"], 16, seed + 1)):
        h, w = Hp // stride, Wp // stride
        base = F.interpolate(seeded((B, ch, 3, 3), s0), size=(h, w), mode="bilinear", align_corners=False)
        feats[key] = base + 0.15 * seeded((B, ch, h, w), s0 + 10)
    inputs = []
    for b, (H, W, oh, ow, kind) in enumerate(cfg["images"]):
        ys, xs = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
        ellipse = ((ys - 0.5) ** 2 / 0.12 + (xs - 0.45) ** 2 / 0.09) < 1.0
        if kind == "ellipse":
            obj = ellipse
        elif kind == "tiny":                       # a 13 x 13 blob around pixel (40, 40): one sample of the stride-8 feature grid
            py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            obj = ((py - 40).abs() <= 6) & ((px - 40).abs() <= 6)
        else:
            obj = torch.zeros_like(ellipse)
        if kind == "tiny":                         # 3 and 10 of the blob's 13 rows: IoUs with the whole blob well away from the thresholds
            parts = torch.stack([obj & (py <= 36), obj & (py > 36)])
        else:                                      # (the image without an object still has ground-truth parts)
            G = 2 + b % 2
            g = torch.Generator().manual_seed(seed + 30 + b)
            centers = torch.rand((G, 2), generator=g) * 0.7 + 0.15
            lab = torch.stack([(ys - c[0]) ** 2 + (xs - c[1]) ** 2 for c in centers]).argmin(0)
            parts = torch.stack([(lab == k) & ellipse for k in range(G)])
        inputs.append({"image": seeded((3, H, W), seed + 20 + b) * 50 + 100, "object_mask": obj[None], "part_masks": parts,
                       "part_labels": torch.arange(parts.shape[0]), "height": oh, "width": ow})
    return feats, inputs


def batched_inputs(inputs, Instances, BitMasks):
    """the model's input dicts from make_pixel_grouping_inputs, built with the package's (or any) Instances / BitMasks classes"""
    out = []
    for i in inputs:
        size = tuple(i["image"].shape[-2:])
        parts, objs = Instances(size), Instances(size)
        parts.gt_masks, parts.gt_classes = BitMasks(i["part_masks"]), i["part_labels"]
        objs.gt_masks, objs.gt_classes = BitMasks(i["object_mask"]), torch.tensor([7])
        out.append({"image": i["image"], "instances": objs, "part_instances": parts, "height": i["height"], "width": i["width"]})
    return out


# ----------------------------------------------------------------------------- host restatement of the boolean mask resize
def axis_taps(n_in, n_out, fused=False):
    """(i0, i1, l1 == 0) of ATen's fp32 bilinear source index (align_corners = False) for every output index, each operation rounded on
    its own; fused: one rounding of the exact scale32 * (d + 0.5) - 0.5 instead (what a fused multiply-add computes)"""
    scale = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out)
    if fused:
        src = (np.float64(scale) * (d.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
    else:
        src = (scale * (d.astype(np.float32) + np.float32(0.5))).astype(np.float32) - np.float32(0.5)
    src = np.maximum(src, np.float32(0))
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (src - i0.astype(np.float32)) == 0


def masks_resize_ref(src, crop, out, fused=False):
    """bool [n, H, W]: bilinear((Hi, Wi) -> (H, W))(src[:, :Hi, :Wi] as float) != 0, from the taps with a non-zero weight"""
    (Hi, Wi), (H, W) = crop, out
    y0, y1, yz = axis_taps(Hi, H, fused)
    x0, x1, xz = axis_taps(Wi, W, fused)
    s = src.cpu().numpy()[:, :Hi, :Wi] != 0
    r0, r1 = s[:, y0], s[:, y1] & ~yz[None, :, None]
    res = r0[:, :, x0] | r1[:, :, x0] | ((r0[:, :, x1] | r1[:, :, x1]) & ~xz[None, None, :])
    return torch.from_numpy(res)
