from .classification_trainer import ClassificationTrainer  # noqa: F401
from .ensemble_trainer import EnsembleTrainer  # noqa: F401
from .layerwise_trainer import LayerwiseTrainer  # noqa: F401
from .taylor_prune_trainer import TaylorPruneTrainer  # noqa: F401
from .analysis_trainer import AnalysisTrainer  # noqa: F401
