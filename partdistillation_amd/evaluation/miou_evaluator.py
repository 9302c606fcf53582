"""``mIOU_Evaluator`` (reference evaluation/miou_evaluator.py): part mIoU / mIoPred / mACC per object class (C-*) and over all
(object class, part) pairs (A-*).

The reference paints a label map per image on the host (one torch.where per mask, later masks win) and np.bincount-s it into a
float64 confusion matrix per object class.  Here process() only launches kernels: the masks are packed into bit planes and the
(predicted label, ground-truth label) pixel counts are added to a dense int64 table [num_object_classes, n + 1, n + 1] on the device,
the row chosen by the image's object class read on the device (no .item()).  evaluate() reads that table once and applies the
reference's formulas (metrics.py) to every object class with any count.

Dataset metadata: class_names (the reference's thing_classes: the A-* lists iterate over them) and gt_num_classes
(len(part_classes), else len(thing_classes)) replace the MetadataCatalog lookup; num_object_classes
(PART_DISTILLATION.NUM_OBJECT_CLASSES) sizes the table.  With several ranks the table is summed with one all_reduce and every rank
returns the same result.  With distributed=False this process's counts are evaluated (the reference returns NaN there: its
per-class loop only runs when distributed)."""
import logging

import torch

from ..functions import eval_metrics as E
from .evaluator import DatasetEvaluator
from .metrics import merge_counts, miou_metrics


def _tensor(x):
    return getattr(x, "tensor", x)


class _ConfusionBase(DatasetEvaluator):
    """dense per-object-class confusion tables over n classes + background, filled on the device"""

    def _setup(self, n, num_object_classes, distributed):
        self.n, self.num_object_classes, self._distributed = int(n), int(num_object_classes), distributed
        self._logger = logging.getLogger("partdistillation_amd.evaluation")
        self.reset()

    def reset(self):
        self._conf = None

    def _table(self, device):
        if self._conf is None:
            self._conf = torch.zeros((self.num_object_classes, self.n + 1, self.n + 1), dtype=torch.int64, device=device)
        return self._conf

    def process(self, inputs, outputs):
        sets, meta = [], []
        for out in outputs:
            pred, gt = out["predictions"], out["gt_instances"]
            pm, gm = _tensor(pred.pred_masks), _tensor(gt.gt_masks)
            if tuple(pm.shape[1:]) != tuple(gm.shape[1:]):
                raise ValueError(f"prediction masks {tuple(pm.shape)} and ground truth {tuple(gm.shape)} disagree")
            slot = out["gt_object_label"]
            if not torch.is_tensor(slot):
                slot = torch.tensor([int(slot)], dtype=torch.int64).to(pm.device, non_blocking=True)
            hw = 1
            for s in pm.shape[1:]:
                hw *= int(s)
            sets += [pm, gm]
            meta.append((pred.pred_classes.long().contiguous(), gt.gt_classes.long().contiguous(), slot.long(), hw))
        if not sets:
            return
        conf = self._table(sets[0].device)
        packed = E.pack_masks(sets)
        E.confusion_add([(p[0], pc, g[0], gc, slot, hw) for p, g, (pc, gc, slot, hw) in zip(packed[0::2], packed[1::2], meta)],
                        self.n, conf)

    def confusion(self):
        """the dense table [num_object_classes, n + 1, n + 1] merged over the ranks, on the host"""
        t = self._conf
        if t is None:
            t = torch.zeros((self.num_object_classes, self.n + 1, self.n + 1), dtype=torch.int64,
                            device="cuda" if torch.cuda.is_available() else "cpu")
        return merge_counts(t.clone(), self._distributed).cpu().numpy()


class mIOU_Evaluator(_ConfusionBase):
    def __init__(self, class_names, gt_num_classes=None, distributed=True, output_dir=None, num_object_classes=1000):
        self._class_names = list(class_names)
        self.gt_num_classes = len(self._class_names) if gt_num_classes is None else int(gt_num_classes)
        self._output_dir = output_dir
        self._setup(self.gt_num_classes, num_object_classes, distributed)

    def evaluate(self):
        return miou_metrics(self.confusion(), self._class_names, self.gt_num_classes)
