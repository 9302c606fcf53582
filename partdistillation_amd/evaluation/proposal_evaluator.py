"""``ProposalEvaluator`` (reference evaluation/proposal_evaluator.py): AR@1 / 10 / 50 / 100 / 200 of the part proposals over the
IoU thresholds 0.50 : 0.05 : 0.95, area range "all".

The reference copies every mask to the host, RLE-encodes it and computes the IoUs with pycocotools in evaluate().  Here process()
only launches kernels (functions/eval_metrics.py): the masks are packed into bit planes, the intersections of the 200 best proposals
with the ground truth are counted, and the greedy cover of every image adds to fixed-size device counters (hits per limit and
threshold, num_pos per limit, images).  evaluate() reads those 56 integers once.

Kept from the reference: proposals in descending score order (a STABLE sort here: equal scores keep their order, the reference's sort
does not promise that); an image without proposals or without ground truth (before the area filter) adds nothing to num_pos; the
area filter of "all" keeps 0 < area <= 1e10; the all-zero placeholder proposal of inference.py counts as a proposal; "# instances" is
the number of images processed.  With several ranks the counters are summed with one all_reduce and only rank 0 returns results.
Limit: at most 64 ground-truth masks per image."""
import logging

import torch

from ..functions import eval_metrics as E
from .evaluator import DatasetEvaluator
from .metrics import is_main_process, merge_counts, proposal_metrics

_NH = len(E.LIMITS) * 10


class ProposalEvaluator(DatasetEvaluator):
    def __init__(self, distributed=True, output_dir=None, areas=("small", "medium", "large", "all"), limit=-1):
        self._logger = logging.getLogger(__name__)
        self._distributed, self._output_dir = distributed, output_dir
        self.areas, self.limit = list(areas), limit
        self.reset()

    def reset(self):
        self._counts = None                     # int64 [5 * 10 hits | 5 num_pos | 1 images] on the device
        self._thr = None

    def _init(self, device):
        if self._counts is None:
            self._counts = torch.zeros(_NH + len(E.LIMITS) + 1, dtype=torch.int64, device=device)
            self._thr = E.thresholds(device)

    def process(self, inputs, outputs):
        sets, kept = [], []
        for out in outputs:
            prop, gt = out["proposals"], out["gt_masks"].gt_masks
            gt = getattr(gt, "tensor", gt)
            self._init(prop.pred_masks.device)
            if prop.pred_masks.shape[0] == 0 or gt.shape[0] == 0:
                continue
            sets += [prop.pred_masks, gt]
            kept.append(torch.sort(prop.scores, descending=True, stable=True)[1][:E.MAX_ROWS].contiguous())
        if len(outputs):
            self._counts[-1] += len(outputs)
        if not kept:
            return
        packed = E.pack_masks(sets)
        pred, gts = packed[0::2], packed[1::2]
        inter = E.intersections([(p[0], order, g[0]) for p, g, order in zip(pred, gts, kept)])
        E.recall_add([(x, order, p[1], g[1]) for x, p, g, order in zip(inter, pred, gts, kept)], self._thr,
                     self._counts[:_NH].view(len(E.LIMITS), 10), self._counts[_NH:_NH + len(E.LIMITS)])

    def counts(self):
        """(hits [5, 10], num_pos [5], images) merged over the ranks, on the host"""
        t = self._counts
        if t is None:
            t = torch.zeros(_NH + len(E.LIMITS) + 1, dtype=torch.int64, device="cuda" if torch.cuda.is_available() else "cpu")
        t = merge_counts(t.clone(), self._distributed).cpu()
        return t[:_NH].view(len(E.LIMITS), 10), t[_NH:_NH + len(E.LIMITS)], int(t[-1])

    def evaluate(self):
        hits, num_pos, images = self.counts()
        if self._distributed and not is_main_process():
            return {}
        if images == 0:
            self._logger.warning("[ProposalEvaluator] Did not receive valid predictions.")
            return {}
        res = proposal_metrics(hits.numpy(), num_pos.numpy(), images)
        self._logger.info("Proposal metrics: %s", res)
        return {"box_proposals": res}
