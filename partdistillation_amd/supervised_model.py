"""``SupervisedModel`` meta-architecture (reference part_distillation/supervised_model.py:30-451): the supervised / few-shot baseline
that proposal learning and part distillation are compared with.  Trained on ground-truth part masks (`part_instances`; labels, or
zeros with CLASS_AGNOSTIC_LEARNING) with the same Hungarian set criterion, evaluated against the same ground truth.

Registered under the reference's name, built from the same config keys (SUPERVISED_MODEL.*), same parameter and buffer names (a
reference state_dict loads), same output contract: in training the weighted loss dict, in evaluation per image
    {"predictions": Instances(pred_masks, pred_classes, scores), "gt_instances": Instances(gt_masks, gt_classes, ...),
     "proposals": <predictions>, "gt_masks": <gt_instances>}
on the device (input of evaluation.Supervised_mIOU_Evaluator / ProposalEvaluator).  The evaluation branch lives in
inference_supervised.py.  Not built: `wandb_visualize`; the iteration counters it is keyed on are kept."""
from typing import Tuple

import torch
from torch import nn

from .compat import META_ARCH_REGISTRY, build_backbone, build_sem_seg_head, configurable
from .proposal_model import _MaskFormerTrainBase, build_criterion


@META_ARCH_REGISTRY.register()
class SupervisedModel(_MaskFormerTrainBase):
    @configurable
    def __init__(self, *, backbone, sem_seg_head: nn.Module, criterion: nn.Module, num_queries: int, num_classes: int,
                 size_divisibility: int, pixel_mean: Tuple[float], pixel_std: Tuple[float], test_topk_per_image: int,
                 dataset_name: str = "", use_wandb: bool = True, wandb_vis_period_train: int = 200, wandb_vis_period_test: int = 5,
                 wandb_vis_topk: int = 200, use_unique_per_pixel_label: bool = False, apply_masking_with_object_mask: bool = True,
                 class_agnostic_learning: bool = True, class_agnostic_inference: bool = False):
        super().__init__()
        self._init_common(backbone, sem_seg_head, criterion, num_queries, num_classes, size_divisibility, pixel_mean, pixel_std)
        self.test_topk_per_image, self.wandb_vis_topk = test_topk_per_image, wandb_vis_topk
        self.use_wandb = use_wandb                                   # accepted for config parity; never used here
        self.wandb_vis_period_train, self.wandb_vis_period_test = wandb_vis_period_train, wandb_vis_period_test
        self.use_unique_per_pixel_label = use_unique_per_pixel_label
        self.apply_masking_with_object_mask = apply_masking_with_object_mask
        self.class_agnostic_learning = class_agnostic_learning
        self.class_agnostic_inference = class_agnostic_inference
        self.num_test_iterations = 0

    @classmethod
    def from_config(cls, cfg):
        backbone = build_backbone(cfg)
        sem_seg_head = build_sem_seg_head(cfg, backbone.output_shape())
        criterion = build_criterion(cfg, sem_seg_head.num_classes)
        sm = cfg.SUPERVISED_MODEL
        return dict(backbone=backbone, sem_seg_head=sem_seg_head, criterion=criterion,
                    num_queries=cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES,
                    size_divisibility=cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY, pixel_mean=cfg.MODEL.PIXEL_MEAN,
                    pixel_std=cfg.MODEL.PIXEL_STD, test_topk_per_image=cfg.TEST.DETECTIONS_PER_IMAGE,
                    wandb_vis_period_train=cfg.WANDB.VIS_PERIOD_TRAIN, wandb_vis_period_test=cfg.WANDB.VIS_PERIOD_TEST,
                    wandb_vis_topk=cfg.WANDB.VIS_TOPK, use_wandb=not cfg.WANDB.DISABLE_WANDB, dataset_name=cfg.DATASETS.TRAIN[0],
                    use_unique_per_pixel_label=sm.USE_PER_PIXEL_LABEL,
                    apply_masking_with_object_mask=sm.APPLY_MASKING_WITH_OBJECT_MASK,
                    class_agnostic_learning=sm.CLASS_AGNOSTIC_LEARNING, class_agnostic_inference=sm.CLASS_AGNOSTIC_INFERENCE,
                    num_classes=cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES)

    def prepare_targets(self, inputs, images):
        """reference :340-365: part masks (`part_instances`) and object masks (`instances`) zero-padded to the batch size; the labels
        are the part classes, or zeros when learning class-agnostically"""
        h_pad, w_pad = images.tensor.shape[-2:]
        out = []
        for x in inputs:
            parts, objs = x["part_instances"].to(self.device), x["instances"].to(self.device)
            pm, om = parts.gt_masks.tensor, objs.gt_masks.tensor
            ppad = torch.zeros((pm.shape[0], h_pad, w_pad), dtype=pm.dtype, device=pm.device)
            ppad[:, : pm.shape[1], : pm.shape[2]] = pm
            opad = torch.zeros((om.shape[0], h_pad, w_pad), dtype=om.dtype, device=om.device)
            opad[:, : om.shape[1], : om.shape[2]] = om
            labels = torch.zeros(pm.shape[0], dtype=torch.long, device=self.device) if self.class_agnostic_learning \
                else parts.gt_classes.to(self.device)
            out.append({"labels": labels, "masks": ppad, "object_masks": opad})
        return out

    def forward(self, batched_inputs):
        images = self.preprocess(batched_inputs)
        targets = self.prepare_targets(batched_inputs, images)
        if not self.training:                                          # evaluation branch (reference :189-198)
            from .inference_supervised import supervised_inference
            outputs = self.sem_seg_head(self.backbone(images.tensor))
            self.num_test_iterations += 1
            return supervised_inference(self, batched_inputs, targets, images, outputs)
        targets = self._share_padded_masks(targets)
        self.criterion.prefetch_num_masks(targets, self.device)
        outputs = self.sem_seg_head(self.backbone(images.tensor))
        losses = self._weighted(self.criterion(outputs, targets))
        self.num_train_iterations += 1
        return losses
