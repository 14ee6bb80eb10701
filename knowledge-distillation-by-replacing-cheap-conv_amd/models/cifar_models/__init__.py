from .resnet import ResNet, resnet20, resnet32, resnet44, resnet56, resnet110  # noqa: F401
from .wrn import WideResNet, wrn  # noqa: F401
from .preresnet import PreResNet, preresnet  # noqa: F401
from .vgg import VGG, make_layers, vgg11, vgg11_bn, vgg13, vgg13_bn, vgg16, vgg16_bn, vgg19, vgg19_bn  # noqa: F401
from .densenet import DenseNet, densenet121, densenet161, densenet169, densenet201  # noqa: F401
