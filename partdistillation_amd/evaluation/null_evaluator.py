"""``NullEvaluator`` (reference evaluation/null_evaluator.py): evaluates nothing; ``evaluate`` waits for the other ranks."""
from .evaluator import DatasetEvaluator


class NullEvaluator(DatasetEvaluator):
    def reset(self):
        return

    def process(self, inputs, outputs):
        return

    def evaluate(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.barrier()
        return
