"""``mIOU_Matcher`` (reference evaluation/miou_matcher.py): the "match" pass of the part-distillation evaluation.  The same device
confusion tables as mIOU_Evaluator, over n = max(gt classes, predicted classes) labels; evaluate() returns, for every object class
seen, the majority-vote mapping predicted part class -> ground-truth part class (argmax over the ground-truth columns, first on ties)
as an int64 tensor on the device, ready for PartDistillationModel.update_majority_vote_mapping.

With several ranks the table is summed with one all_reduce and every rank returns the same mapping.  With distributed=False this
process's counts are used (the reference returns an empty mapping there)."""
import torch

from .metrics import majority_voting, seen_slots
from .miou_evaluator import _ConfusionBase


class mIOU_Matcher(_ConfusionBase):
    def __init__(self, class_names, gt_num_classes=None, num_classes=8, distributed=True, num_object_classes=1000):
        self._class_names = list(class_names)
        self.gt_num_classes = len(self._class_names) if gt_num_classes is None else int(gt_num_classes)
        self.pred_num_classes = int(num_classes)
        self._setup(max(self.gt_num_classes, self.pred_num_classes), num_object_classes, distributed)

    def evaluate(self):
        conf = self.confusion()
        device = self._conf.device if self._conf is not None else torch.device("cpu")
        return {k: majority_voting(conf[k], self.pred_num_classes, self.gt_num_classes).to(device) for k in seen_slots(conf)}
