"""`EnsembleStudent` (reference models/students/ensemble_student.py:10-16): a DepthwiseStudent with an (empty) list for member
networks.  The attribute's spelling is the reference's; EnsembleTrainer keeps its members in `trainer.models`, as the reference does."""
from torch import nn

from .depthwise_student import DepthwiseStudent


class EnsembleStudent(DepthwiseStudent):
    def __init__(self, teacher_model, config):
        super().__init__(teacher_model, config)
        self.studdents = nn.ModuleList()
