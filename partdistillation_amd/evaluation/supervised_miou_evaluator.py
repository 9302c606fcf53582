"""``Supervised_mIOU_Evaluator`` (reference evaluation/supervised_miou_evaluator.py): part mIoU / mACC / mIoPred of SupervisedModel's
predictions over ONE confusion table of num_classes classes + background.

The reference paints a label map per image on the host (one torch.where per mask, later masks win, fill = num_classes) and
np.bincount-s it into a float64 matrix.  Here process() only launches kernels: the masks are packed into bit planes and
pd_eval_confusion_grouped adds the (predicted label, ground-truth label) pixel counts to an int64 table [1, n + 1, n + 1] on the
device (one slot).  evaluate() reads that table once, sums it over the ranks with one all_reduce when a process group exists, and
applies the reference's measure_mIOU in float64 on the host (metrics.supervised_miou_metrics).

`dataset_name_or_class_names`: the class names (the reference's MetadataCatalog.get(dataset_name).thing_classes), or a dataset name
for which names "0" .. "num_classes - 1" are used.  With distributed=False the reference averages empty lists and returns NaN; this
evaluator uses the local table there."""
import torch

from .metrics import supervised_miou_metrics
from .miou_evaluator import _ConfusionBase


class Supervised_mIOU_Evaluator(_ConfusionBase):
    def __init__(self, dataset_name_or_class_names, num_classes=8, distributed=True, output_dir=None):
        if isinstance(dataset_name_or_class_names, str):
            self._dataset_name, self._class_names = dataset_name_or_class_names, [str(i) for i in range(num_classes)]
        else:
            self._dataset_name, self._class_names = "", list(dataset_name_or_class_names)
        self._num_classes, self._output_dir = int(num_classes), output_dir
        self._slot = None
        self._setup(self._num_classes, 1, distributed)

    def process(self, inputs, outputs):
        if outputs and self._slot is None:                             # every image counts in the one table: slot 0, made once
            dev = outputs[0]["predictions"].pred_masks.device
            self._slot = torch.zeros(1, dtype=torch.int64, device=dev)
        super().process(inputs, [dict(o, gt_object_label=self._slot) for o in outputs])

    def evaluate(self):
        return supervised_miou_metrics(self.confusion()[0], self._class_names, self._num_classes)
