"""``inference_on_dataset`` (detectron2.evaluation.evaluator.inference_on_dataset): reset the evaluator, run the model in eval
mode under torch.no_grad over the loader, hand every batch to ``process``, ``evaluate`` at the end, restore the training mode."""
import torch


class DatasetEvaluator:
    """the reset / process / evaluate contract of detectron2's DatasetEvaluator"""

    def reset(self):
        pass

    def process(self, inputs, outputs):
        pass

    def evaluate(self):
        pass


class DatasetEvaluators(DatasetEvaluator):
    """several evaluators as one; their result dicts are merged (a key may come from one evaluator only)"""

    def __init__(self, evaluators):
        self._evaluators = list(evaluators)

    def reset(self):
        for e in self._evaluators:
            e.reset()

    def process(self, inputs, outputs):
        for e in self._evaluators:
            e.process(inputs, outputs)

    def evaluate(self):
        results = {}
        for e in self._evaluators:
            for k, v in (e.evaluate() or {}).items():
                if k in results:
                    raise KeyError(f"two evaluators returned the key {k!r}")
                results[k] = v
        return results


def inference_on_dataset(model, data_loader, evaluator):
    """model(inputs) -> outputs for every batch of data_loader, evaluator.process(inputs, outputs); returns evaluator.evaluate()
    ({} when it returns None).  evaluator may be None (nothing is evaluated) or a list of evaluators."""
    if evaluator is None:
        evaluator = DatasetEvaluators([])
    elif isinstance(evaluator, (list, tuple)):
        evaluator = DatasetEvaluators(evaluator)
    evaluator.reset()
    was_training = getattr(model, "training", False)
    if hasattr(model, "eval"):
        model.eval()
    try:
        with torch.no_grad():
            for inputs in data_loader:
                outputs = model(inputs)
                evaluator.process(inputs, outputs)
    finally:
        if hasattr(model, "train"):
            model.train(was_training)
    results = evaluator.evaluate()
    return {} if results is None else results
