"""CIFAR pre-activation ResNet (He et al., "Identity Mappings in Deep Residual Networks"; preresnet-110 is the CIFAR-100 teacher
whose weights the reference's authors left in checkpoints/cifar100/preresnet-110.pth) with the reference's module tree and
state-dict keys (models/cifar_models/preresnet.py): conv1, layer{1,2,3}.{i}.{bn1, conv1, bn2, conv2[, bn3, conv3], downsample.0},
bn, fc -- so a checkpoint loads through forgiving_state_restore.  Same initialisation rule.

Both block types are pre-activation: every conv reads relu(bn(.)) of its input.  The stride sits on conv1 of a BasicBlock and on
the 3x3 conv2 of a Bottleneck.  Where stride or width changes (the first block of a layer) the shortcut is a bare 1x1 conv with the
block's stride and no BN that reads the RAW block input, not the activated one; everywhere else it is the input itself.

Channels-last fp32 throughout, as in wrn.py: the convs are nn_hip.Conv2dNHWC, the BatchNorms nn_hip.BatchNorm2dNHWC, and the
residual add rides in the last conv's epilogue.  Under autograd bn1 of every block is taken with forward_with_shortcut, so the
shortcut's gradient joins dx inside the BN backward kernel.  The tail bn -> relu -> 8x8 average pool is one kernel that never stores
the activation (nn_hip.bn_relu_avgpool, csrc/head_ops.hip); the 64 * expansion -> classes linear layer is a torch op.

Eval mode without autograd (the frozen teacher, validation) runs a block as one launch per conv: each conv's epilogue applies the
next BN (folded to scale / shift) + ReLU, the last conv adds the shortcut and writes both the block output and the next block's
relu(bn1(.)) of it; the last block of the network writes its raw output only, which the head reads.  That fusion needs the block's
children to be the nn_hip classes without hooks; a block holding a DepthwiseSeparableBlock calls its children as modules.  Hooks on
block or layer names see the block output either way.  fp32 only.
"""
import math

import torch
import torch.nn as nn

from ... import nn_hip
from ...nn_hip import BatchNorm2dNHWC, Conv2dNHWC, _nhwc

__all__ = ["preresnet", "PreResNet"]

_ACT = "_preresnet_act"    # block output -> (the BN it was activated with, relu(bn(output))) of the fused eval chain


def _take_act(x, bn):
    """The activation the producing block stored for `bn`, if any; the attribute is dropped once read, so a stored block output
    (a hint) does not keep it alive."""
    a = getattr(x, _ACT, None)
    if a is None:
        return None
    delattr(x, _ACT)
    return a[1] if a[0] is bn else None


class _PreActBlock(nn.Module):
    """bn_i -> relu -> conv_i for every stage of the subclass, plus the shortcut.  Subclasses create the children (in the
    reference's order, which is the state dict's) and name their stages."""

    def _stages(self):
        raise NotImplementedError

    def _bn_relu(self, bn, x):
        """relu(bn(x)) as a module call; the nn_hip BatchNorms fuse the ReLU into their kernel."""
        return bn(x, relu=True) if isinstance(bn, (nn_hip.BatchNorm2dNHWC, nn_hip.BatchNorm2d)) else self.relu(bn(x))

    def _fusable(self, x):
        bns, convs = self._stages()
        short = () if self.downsample is None else tuple(self.downsample)
        return (x.is_cuda and x.dtype == torch.float32 and not self.training and not torch.is_grad_enabled()
                and all(type(c) is nn_hip.Conv2dNHWC for c in convs + short) and all(type(b) is nn_hip.BatchNorm2dNHWC for b in bns)
                and len(short) <= 1 and not nn_hip._hooked(self.relu, *bns, *convs, *short)
                and (self.downsample is None or not nn_hip._hooked(self.downsample)))

    def _forward_fused(self, x):
        bns, convs = self._stages()
        a = _take_act(x, bns[0])
        if a is None:
            a = bns[0](x, relu=True)
        if self.downsample is None:
            sc = _nhwc(x)
        else:
            ds = self.downsample[0]
            ds._check()
            sc = ds._run(ds._input(x))
        for conv, bn in zip(convs[:-1], bns[1:]):
            conv._check()
            s, b = bn.folded()
            _, a = conv._run(conv._input(a), out_act=True, act_scale=s, act_shift=b, act_relu=True, want_raw=False, act_padded=True)
            a = nn_hip.mark_padded(a.permute(0, 3, 1, 2))
        last = convs[-1]
        last._check()
        nxt = self._next[0]
        if nxt is None or type(nxt) is not nn_hip.BatchNorm2dNHWC or nn_hip._hooked(nxt):
            return last._run(last._input(a), res_pre=sc).permute(0, 3, 1, 2)
        s, b = nxt.folded()
        raw, act = last._run(last._input(a), res_pre=sc, out_act=True, act_scale=s, act_shift=b, act_relu=True, act_padded=True)
        out = raw.permute(0, 3, 1, 2)
        setattr(out, _ACT, (nxt, nn_hip.mark_padded(act.permute(0, 3, 1, 2))))
        return out

    def forward(self, x):
        if self._fusable(x):
            return self._forward_fused(x)
        bns, convs = self._stages()
        if type(bns[0]) is nn_hip.BatchNorm2dNHWC and not nn_hip._hooked(bns[0]):
            out, x = bns[0].forward_with_shortcut(x, relu=True)      # the shortcut's gradient joins bn1's dx in its kernel
        else:
            out = self._bn_relu(bns[0], x)
        for conv, bn in zip(convs[:-1], bns[1:]):
            out = self._bn_relu(bn, conv(out))
        sc = x if self.downsample is None else self.downsample(x)    # (the raw block input, not relu(bn1(x)))
        if isinstance(convs[-1], nn_hip.Conv2dNHWC):
            return convs[-1](out, residual=sc)
        return torch.add(sc, convs[-1](out))


class BasicBlock(_PreActBlock):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.bn1 = BatchNorm2dNHWC(inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.conv1 = Conv2dNHWC(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = BatchNorm2dNHWC(planes)
        self.conv2 = Conv2dNHWC(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.downsample = downsample
        self.stride = stride
        self._next = (None,)     # the BN that reads this block's output (PreResNet sets it; a tuple, not a child module)

    def _stages(self):
        return (self.bn1, self.bn2), (self.conv1, self.conv2)


class Bottleneck(_PreActBlock):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.bn1 = BatchNorm2dNHWC(inplanes)
        self.conv1 = Conv2dNHWC(inplanes, planes, kernel_size=1, bias=False)
        self.bn2 = BatchNorm2dNHWC(planes)
        self.conv2 = Conv2dNHWC(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn3 = BatchNorm2dNHWC(planes)
        self.conv3 = Conv2dNHWC(planes, planes * 4, kernel_size=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self._next = (None,)

    def _stages(self):
        return (self.bn1, self.bn2, self.bn3), (self.conv1, self.conv2, self.conv3)


class PreResNet(nn.Module):
    def __init__(self, depth, num_classes=1000, block_name="BasicBlock"):
        super().__init__()
        if block_name.lower() == "basicblock":
            assert (depth - 2) % 6 == 0, "a BasicBlock PreResNet has depth 6n+2 (20, 32, 44, 56, 110, 1202)"
            n, block = (depth - 2) // 6, BasicBlock
        elif block_name.lower() == "bottleneck":
            assert (depth - 2) % 9 == 0, "a Bottleneck PreResNet has depth 9n+2 (20, 29, 47, 56, 110, 164, 1001)"
            n, block = (depth - 2) // 9, Bottleneck
        else:
            raise ValueError("block_name is BasicBlock or Bottleneck")
        self.inplanes = 16
        self.conv1 = Conv2dNHWC(3, 16, kernel_size=3, padding=1, bias=False)
        self.layer1 = self._make_layer(block, 16, n, 1)
        self.layer2 = self._make_layer(block, 32, n, 2)
        self.layer3 = self._make_layer(block, 64, n, 2)
        self.bn = BatchNorm2dNHWC(64 * block.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.avgpool = nn.AvgPool2d(8)
        self.fc = nn.Linear(64 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / fan))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
        blocks = [b for layer in (self.layer1, self.layer2, self.layer3) for b in layer]
        for b, nxt in zip(blocks, [b.bn1 for b in blocks[1:]] + [None]):      # (the last block writes its raw output only: the head reads it)
            b._next = (nxt,)

    def _make_layer(self, block, planes, blocks, stride):
        width = planes * block.expansion
        downsample = None
        if stride != 1 or self.inplanes != width:
            downsample = nn.Sequential(Conv2dNHWC(self.inplanes, width, kernel_size=1, stride=stride, bias=False))
        layers = [block(self.inplanes, planes, stride, downsample)] + [block(width, planes) for _ in range(1, blocks)]
        self.inplanes = width
        return nn.Sequential(*layers)

    def forward(self, x):
        out = self.layer3(self.layer2(self.layer1(self.conv1(x))))
        if getattr(out, _ACT, None) is not None:       # (a block that was told of no head BN leaves none; a stale tag is dropped)
            delattr(out, _ACT)
        ks = self.avgpool.kernel_size
        out = nn_hip.bn_relu_avgpool(self.bn, self.relu, out, ks if isinstance(ks, int) else ks[0])
        return self.fc(out)


def preresnet(**kwargs):
    """Constructs a CIFAR pre-activation ResNet (depth, num_classes, block_name)."""
    return PreResNet(**kwargs)
