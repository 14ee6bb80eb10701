"""CIFAR VGG (Simonyan & Zisserman's configurations A, B, D, E with the fully connected layers removed: the 512-channel 1x1 map
of a 32x32 input goes straight to one linear layer), with or without BatchNorm, with the reference's module tree and state-dict keys
(models/cifar_models/vgg.py): `features` is an nn.Sequential (the subclass Features) of conv, [bn,] relu and max-pool children
under the reference's indices -- features.{i}.weight / bias / running_* -- and `classifier` the linear layer, so a checkpoint loads through
forgiving_state_restore and every `features.N` name of a pruning plan resolves.  Same initialisation rule.

Channels-last fp32 throughout: the convs are biased nn_hip.Conv2dNHWC, the BatchNorms nn_hip.BatchNorm2dNHWC.  Features.forward does
not call its children one by one; it walks them in groups  conv [bn] relu [pool]:
  * under autograd a group that ends in a pool takes its tail through nn_hip.bn_relu_maxpool -- BatchNorm, ReLU and MaxPool2d(2, 2)
    as one kernel that reads the conv output once and stores the pooled map only (csrc/pool_ops.hip) --, a group without a pool
    takes bn(x, relu=True) (the plain nets, which have no BatchNorm to fuse it into, take torch.relu);
  * eval mode without autograd (the frozen teacher, validation) is one launch per conv: its epilogue adds the bias and applies the
    folded BatchNorm and the ReLU, and a pooled group then runs the no-BatchNorm form of the pool kernel on the activated map.
A forward hook on any member of a group, or a member that is not the class this file put there (a DepthwiseSeparableBlock in place
of a conv), makes that group call its children as modules; a hook on a conv sees the conv's output (bias added) either way, one
on `features` the 512-channel 1x1 map.
fp32 only.
"""
import math

import torch
import torch.nn as nn

from ... import nn_hip
from ...nn_hip import BatchNorm2dNHWC, Conv2dNHWC

__all__ = ["VGG", "make_layers", "vgg11", "vgg11_bn", "vgg13", "vgg13_bn", "vgg16", "vgg16_bn", "vgg19_bn", "vgg19"]


class Features(nn.Sequential):
    """The `features` of a VGG: an nn.Sequential (same children, same keys) whose forward walks the children in groups
    conv [bn] relu [pool] as the module docstring says, instead of one by one."""

    def __init__(self, *args):
        super().__init__(*args)
        self._identity = {}

    def __deepcopy__(self, memo):
        return nn_hip._deepcopy_without(self, memo, _identity={})

    def groups(self):
        """The children as (head, bn | None, relu | None, pool | None): a head (a conv, or whatever stands in its place) and the
        BatchNorm, ReLU and MaxPool2d that follow it, in that order, as far as they are there."""
        mods, groups, i = list(self), [], 0
        while i < len(mods):
            group = [mods[i], None, None, None]
            i += 1
            for slot, kind in ((1, nn.BatchNorm2d), (2, nn.ReLU), (3, nn.MaxPool2d)):
                if i < len(mods) and isinstance(mods[i], kind):
                    group[slot] = mods[i]
                    i += 1
            groups.append(tuple(group))
        return groups

    def _scale_shift(self, conv, bn, device):
        """What the conv's epilogue applies before its ReLU: the folded eval-mode BatchNorm, or the identity."""
        if bn is not None:
            return bn.folded()
        key = (conv.out_channels, device)
        if key not in self._identity:
            self._identity[key] = (torch.ones(conv.out_channels, device=device), torch.zeros(conv.out_channels, device=device))
        return self._identity[key]

    def _fusable(self, x, conv, bn, relu, pool):
        mods = [m for m in (conv, bn, relu, pool) if m is not None]
        return (x.is_cuda and not torch.is_grad_enabled() and type(conv) is Conv2dNHWC and type(relu) is nn.ReLU
                and (bn is None or (type(bn) is BatchNorm2dNHWC and not bn.training))
                and (pool is None or (nn_hip._plain_maxpool2x2(pool) and x.shape[2] >= 2 and x.shape[3] >= 2))
                and not nn_hip._hooked(*mods))

    def _group(self, x, conv, bn, relu, pool):
        if relu is None:                                   # (not a layout make_layers produces: the children as they stand)
            for m in (conv, bn, pool):
                x = x if m is None else m(x)
            return x
        if self._fusable(x, conv, bn, relu, pool):
            conv._check()
            s, b = self._scale_shift(conv, bn, x.device)
            _, a = conv._run(conv._input(x), out_act=True, act_scale=s, act_shift=b, act_relu=True, want_raw=False, act_padded=True)
            a = nn_hip.mark_padded(a.permute(0, 3, 1, 2))
            return a if pool is None else nn_hip.bn_relu_maxpool(None, relu, pool, a)
        x = conv(x)
        if pool is not None:
            return nn_hip.bn_relu_maxpool(bn, relu, pool, x)
        if not x.is_cuda:
            return relu(x if bn is None else bn(x))
        if bn is None:                                     # (no BatchNorm kernel to fuse it into: an elementwise torch op)
            return nn_hip.call_relu(relu, x) if nn_hip._hooked(relu) or type(relu) is not nn.ReLU else torch.relu(x)
        if isinstance(bn, (nn_hip.BatchNorm2dNHWC, nn_hip.BatchNorm2d)) and not nn_hip._hooked(relu):
            return bn(x, relu=True)
        return nn_hip.call_relu(relu, bn(x))

    def forward(self, x):
        for group in self.groups():
            x = self._group(x, *group)
        return x


class VGG(nn.Module):
    def __init__(self, features, num_classes=1000):
        super().__init__()
        self.features = Features(*features) if type(features) is nn.Sequential else features
        self.classifier = nn.Linear(512, num_classes)
        self._initialize_weights()

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / fan))
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                m.weight.data.normal_(0, 0.01)
                m.bias.data.zero_()

    def forward(self, x):
        if x.dtype != torch.float32:
            raise TypeError("VGG is fp32")
        x = self.features(x)
        return self.classifier(x.reshape(x.size(0), -1))


def make_layers(cfg, batch_norm=False):
    """cfg: output channels of a 3x3 conv (padding 1, biased), or 'M' for MaxPool2d(2, 2); every conv is followed by
    [BatchNorm,] ReLU."""
    layers, in_channels = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        layers.append(Conv2dNHWC(in_channels, v, kernel_size=3, padding=1, bias=True))
        if batch_norm:
            layers.append(BatchNorm2dNHWC(v))
        layers.append(nn.ReLU(inplace=True))
        in_channels = v
    return Features(*layers)


cfg = {
    "A": [64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    "B": [64, 64, "M", 128, 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    "D": [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"],
    "E": [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"],
}


def vgg11(**kwargs):
    """VGG 11-layer model (configuration "A")"""
    return VGG(make_layers(cfg["A"]), **kwargs)


def vgg11_bn(**kwargs):
    """VGG 11-layer model (configuration "A") with batch normalization"""
    return VGG(make_layers(cfg["A"], batch_norm=True), **kwargs)


def vgg13(**kwargs):
    """VGG 13-layer model (configuration "B")"""
    return VGG(make_layers(cfg["B"]), **kwargs)


def vgg13_bn(**kwargs):
    """VGG 13-layer model (configuration "B") with batch normalization"""
    return VGG(make_layers(cfg["B"], batch_norm=True), **kwargs)


def vgg16(**kwargs):
    """VGG 16-layer model (configuration "D")"""
    return VGG(make_layers(cfg["D"]), **kwargs)


def vgg16_bn(**kwargs):
    """VGG 16-layer model (configuration "D") with batch normalization"""
    return VGG(make_layers(cfg["D"], batch_norm=True), **kwargs)


def vgg19(**kwargs):
    """VGG 19-layer model (configuration "E")"""
    return VGG(make_layers(cfg["E"]), **kwargs)


def vgg19_bn(**kwargs):
    """VGG 19-layer model (configuration "E") with batch normalization"""
    return VGG(make_layers(cfg["E"], batch_norm=True), **kwargs)
