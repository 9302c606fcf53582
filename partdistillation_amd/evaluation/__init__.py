from .clustering_module import ClusteringModule  # noqa: F401
from .evaluator import DatasetEvaluator, DatasetEvaluators, inference_on_dataset  # noqa: F401
from .miou_evaluator import mIOU_Evaluator  # noqa: F401
from .miou_matcher import mIOU_Matcher  # noqa: F401
from .null_evaluator import NullEvaluator  # noqa: F401
from .proposal_evaluator import ProposalEvaluator  # noqa: F401
from .supervised_miou_evaluator import Supervised_mIOU_Evaluator  # noqa: F401
