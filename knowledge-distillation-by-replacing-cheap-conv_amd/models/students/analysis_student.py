"""`AnalysisStudent`: the layer-compressibility probe (models/students/analysis_student.py:9-44 of the reference).  A probed
3x3 block is replaced by Sequential(frozen copy of the teacher block, RandomMask2d, trainable bias-free 1x1): how well a 1x1
rebuilds the block's output from a random 15 % of its filters says how redundant the layer is.  Inside a DeepWV3Plus / GSCNN
student the engine runs the Sequential as ONE masked site: the frozen conv computes the kept filters only (engine._Site)."""
import copy
import gc

from torch import nn

from .depthwise_student import DepthwiseStudent
from .transform_blocks import RandomMask2d


class AnalysisStudent(DepthwiseStudent):
    def replace(self, block_names, **kwargs):
        """block_names: list of block names (strings, unlike DepthwiseStudent.replace's dicts); droprate=: RandomMask2d's rate."""
        droprate = kwargs['droprate']
        ref = next(self.student.parameters())
        for block_name in block_names:
            self.replaced_block_names.append(block_name)
            teacher_block = self.get_block(block_name, self.teacher)
            cp_teacher_block = copy.deepcopy(teacher_block).float()      # frozen, like its source (the 1x1 alone trains)
            for p in cp_teacher_block.parameters():
                p.requires_grad = False
            replace_block = nn.Sequential(cp_teacher_block,
                                          RandomMask2d(teacher_block.out_channels, droprate),
                                          nn.Conv2d(teacher_block.out_channels, teacher_block.out_channels, kernel_size=1, bias=False))
            replace_block.to(ref.device)
            self._set_block(block_name, replace_block, self.student)
        if self._engine is not None:
            self._engine.drop_caches()   # the replaced conv's packed weights must not outlive it
        gc.collect()
