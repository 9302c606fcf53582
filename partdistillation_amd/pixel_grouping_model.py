"""Pixel-grouping proposals scored against ground-truth parts (reference pixel_grouping_model.py:28-218; the evaluation twin of
proposal_generation_model.py): backbone features of the object's pixels are clustered into K groups, every object pixel of the
OUTPUT-resolution image is labelled with its nearest centroid, and the per-label masks are returned as proposals next to the ground-truth
part masks — the input of evaluation.ProposalEvaluator (AR@k of a backbone's grouping before any training run).

Same class name / registry / constructor arguments / config keys / output contract as the reference:
    [{"proposals": Instances(pred_masks bool [P, H, W], scores ones [P]), "gt_masks": Instances(gt_masks = pred_masks = bool [G, H, W])}]
on the device.  What is done differently:
  * evaluation mappers resize the image, so (height, width) differ from the size the network saw and every full-resolution map goes
    through sem_seg_postprocess (crop the padding, second bilinear resize).  The reference does that to the C-channel features; here the
    K score maps are formed at feature resolution and pd_scores_argmax_resized_u8 applies BOTH interpolations while writing the uint8
    label map, one launch per batch (include/pd_grouping.h);
  * `sem_seg_postprocess(masks).bool()` of the object mask and of the ground-truth part masks is pd_masks_resize_u8: no float image;
  * K-means runs on the device (functions/kmeans.py); the labels present in each image (the reference's `unique()`) come from the label
    kernel's counts, one device -> host copy per batch;
  * `scores` are float32 ones (the reference's `new_ones` of a bool tensor yields bool ones; sorting and comparing treat them alike).
Not built: `wandb_visualize` (the reference logs the first image of every VIS_PERIOD_TEST-th batch to wandb); the iteration counter it
is keyed on, `num_test_iterations`, is kept."""
from typing import List, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .compat import META_ARCH_REGISTRY, ImageList, Instances, build_backbone, configurable
from .functions import pixel_grouping as G
from .functions.kmeans import kmeans_lloyd_batched
from .proposal_generation_model import ProposalGenerationModel


@META_ARCH_REGISTRY.register()
class PixelGroupingModel(nn.Module):
    @configurable
    def __init__(self, *, backbone, size_divisibility: int, pixel_mean: Tuple[float], pixel_std: Tuple[float], distance_metric: str = "l2",
                 backbone_feature_key_list: List[str] = ("res4",), num_superpixel_clusters: int = 4, feature_normalize: bool = False,
                 debug: bool = False, object_mask_type: str = "detic_based", wandb_vis_period: int = 100):
        super().__init__()
        assert distance_metric in ("dot", "l2")
        assert 1 <= num_superpixel_clusters <= G.MAX_K
        self.backbone = backbone
        if size_divisibility < 0:
            size_divisibility = self.backbone.size_divisibility
        self.size_divisibility = size_divisibility
        self.register_buffer("pixel_mean", torch.Tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.Tensor(pixel_std).view(-1, 1, 1), False)
        self.distance_metric = distance_metric
        self.backbone_feature_key_list = list(backbone_feature_key_list)
        self.num_superpixel_clusters = num_superpixel_clusters
        self.feature_normalize = feature_normalize
        self.debug, self.object_mask_type, self.wandb_vis_period = debug, object_mask_type, wandb_vis_period
        self.num_test_iterations = 0
        self.kmeans_generator = None               # torch.Generator for the k-means++ seeding (None = global device RNG)
        self.init_centroids = None                 # test hook: callable(image index) -> [K,C] initial centres
        self.debug_last = None                     # PIXEL_GROUPING.DEBUG: centroids / resized object masks / label maps of the last batch

    @classmethod
    def from_config(cls, cfg):
        pg = cfg.PIXEL_GROUPING
        return {"backbone": build_backbone(cfg), "size_divisibility": cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY,
                "pixel_mean": cfg.MODEL.PIXEL_MEAN, "pixel_std": cfg.MODEL.PIXEL_STD, "distance_metric": pg.DISTANCE_METRIC,
                "backbone_feature_key_list": pg.BACKBONE_FEATURE_KEY_LIST, "num_superpixel_clusters": pg.NUM_SUPERPIXEL_CLUSTERS,
                "feature_normalize": pg.FEATURE_NORMALIZE, "wandb_vis_period": cfg.WANDB.VIS_PERIOD_TEST, "debug": pg.DEBUG}

    @property
    def device(self):
        return self.pixel_mean.device

    # shared with the generation model: feature concatenation / normalisation and the [K, h, w] score maps
    _prepare_features = ProposalGenerationModel._prepare_features
    _scores = ProposalGenerationModel._scores

    def prepare_mask(self, inputs):
        """un-padded bool masks per image (reference :88-110 pads them to the batch size and sem_seg_postprocess crops the padding off
        again; the resize kernel takes the crop as it is): the FIRST object mask [1, Hi, Wi] and the part masks [G, Hi, Wi]"""
        out = []
        for x in inputs:
            obj = x["instances"].to(self.device).gt_masks.tensor
            parts = x["part_instances"].to(self.device).gt_masks.tensor
            assert obj.shape[0] >= 1, "pixel grouping needs the object mask of every image"
            out.append({"masks": obj[:1].bool(), "part_masks": parts.bool()})
        return out

    # ------------------------------------------------------------------ forward (reference :129-179)
    @torch.no_grad()
    def forward(self, batched_inputs):
        assert not self.training, "pixel grouping is eval only."
        images = [(x["image"].to(self.device) - self.pixel_mean) / self.pixel_std for x in batched_inputs]
        images = ImageList.from_tensors(images, self.size_divisibility)
        targets = self.prepare_mask(batched_inputs)
        backbone_out = self.backbone(images.tensor)               # may run under the caller's autocast
        with torch.autocast(device_type=self.device.type, enabled=False):
            return self._group(batched_inputs, images, targets, self._prepare_features(backbone_out))

    def _group(self, batched_inputs, images, targets, features):
        """clustering + labelling, always fp32 (the kernels take fp32 score maps)"""
        Hp, Wp = images.tensor.shape[-2:]
        K = self.num_superpixel_clusters
        sizes = [(inp.get("height", sz[0]), inp.get("width", sz[1])) for inp, sz in zip(batched_inputs, images.image_sizes)]
        # object mask and ground-truth part masks at output resolution: one launch for the batch
        resize = []
        for tgt, isz, osz in zip(targets, images.image_sizes, sizes):
            resize += [(tgt["masks"], isz, osz), (tgt["part_masks"], isz, osz)]
        resized = G.masks_resize(resize)
        obj_resized, gt_resized = [r[0][0] for r in resized[0::2]], [r[0] for r in resized[1::2]]
        # object pixels at feature resolution (nearest resize of the padded mask), centroids of the images with more than K of them
        datas, inits, slot = [], [], []
        for i, (feat, tgt, isz) in enumerate(zip(features, targets, images.image_sizes)):
            padded = F.pad(tgt["masks"][None].float(), (0, Wp - isz[1], 0, Hp - isz[0]))
            mask_low = F.interpolate(padded, size=feat.shape[-2:], mode="nearest")[0, 0].bool()
            data = feat[:, mask_low].t().contiguous()                                      # [N, C]
            slot.append(len(datas) if data.shape[0] > K else None)
            if slot[-1] is not None:
                datas.append(data)
                inits.append(self.init_centroids(i) if self.init_centroids is not None else None)
        centroids = kmeans_lloyd_batched(datas, K, inits=inits, generator=self.kmeans_generator)[0] if datas else None
        # label maps: an image with K or fewer object pixels has the reference's single all-zero centroid (:190-191) — one constant score map
        items = []
        for feat, s, m, isz in zip(features, slot, obj_resized, images.image_sizes):
            scores = self._scores(feat, centroids[s]) if s is not None else feat.new_zeros((1,) + tuple(feat.shape[-2:]), dtype=torch.float32)
            items.append((scores, m, (Hp, Wp), isz))
        labels, counts = G.scores_argmax_resized(items)
        counts = counts.cpu()                                                              # the batch's only device -> host copy here
        results = []
        for lab, cnt, gt, (H, W) in zip(labels, counts.tolist(), gt_resized, sizes):
            present = [l for l in range(1, len(cnt)) if cnt[l] > 0]                        # ascending: the reference's unique()
            pred = torch.stack([lab == l for l in present]) if present else lab.new_zeros((0, H, W), dtype=torch.bool)
            prop = Instances((H, W))
            prop.pred_masks = pred
            prop.scores = torch.ones(len(present), dtype=torch.float32, device=lab.device)
            gti = Instances((H, W))
            gti.gt_masks = gt
            gti.pred_masks = gt
            results.append({"proposals": prop, "gt_masks": gti})
        if self.debug:                                                                     # intermediate results of the last batch
            self.debug_last = {"centroids": [centroids[s] if s is not None else None for s in slot], "object_masks": obj_resized,
                               "labels": labels, "counts": counts}
        self.num_test_iterations += 1
        return results
