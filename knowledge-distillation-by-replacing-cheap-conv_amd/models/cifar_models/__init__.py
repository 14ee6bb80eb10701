from .resnet import ResNet, resnet20, resnet32, resnet44, resnet56, resnet110  # noqa: F401
from .wrn import WideResNet, wrn  # noqa: F401
from .preresnet import PreResNet, preresnet  # noqa: F401
from .densenet import DenseNet, densenet121, densenet161, densenet169, densenet201  # noqa: F401
