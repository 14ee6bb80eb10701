"""CIFAR Wide-ResNet (Zagoruyko & Komodakis; WRN-28-10 is the teacher of cfg/cifar100/wrn_28_10/config1-7.json) with the
reference's module tree and state-dict keys (models/cifar_models/wrn.py): conv1, block{1,2,3}.layer.{i}.{bn1, relu1, conv1, bn2,
relu2, conv2, convShortcut}, bn1, relu, fc -- so a checkpoint loads through forgiving_state_restore.  Same initialisation rule.

Channels-last throughout: the image is laid out NHWC by the stem conv, every later tensor is an NCHW-logical view with NHWC
strides.  Convolutions are nn_hip.Conv2dNHWC (MFMA implicit GEMM) and BatchNorm nn_hip.BatchNorm2dNHWC (kd_bn_nhwc_*);
the residual add rides in conv2's epilogue.  The 8x8 average pool and the 640 -> classes linear layer are torch ops (like the
ResNet path's `linear`).

The activation dtype is the input's: fp32, or bf16 (a bf16 channels-last batch runs every conv and BN in bf16 with fp32 parameters,
through both paths below; the last bn1 + ReLU output is cast to fp32 before the pool, so the logits are fp32 either way).  In bf16
the convs' K granule is 64 channels: the 16- and 160-channel tensors live in buffers zero-padded to 64 / 192 (nn_hip.new_padded).

Eval mode without autograd (the frozen teacher, validation) runs a block as two conv launches: conv1's epilogue applies bn2 +
ReLU (folded to scale / shift), conv2's adds the shortcut and writes both the block output and the next BN + ReLU of it.  That
fusion needs both convs of the block to be Conv2dNHWC; a block holding a DepthwiseSeparableBlock calls its children as modules.
Hooks on block or group names see the block output either way.

dropRate > 0: in train mode a block drops relu2(bn2(conv1)) before conv2 (the reference's F.dropout), in either dtype, with one
nn_hip.dropout pass (kd_dropout_nhwc: a counter-based mask the backward regenerates, nothing stored); eval mode is unchanged.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import nn_hip
from ...nn_hip import BatchNorm2dNHWC, Conv2dNHWC, _nhwc

__all__ = ["wrn", "WideResNet"]

_ACT = "_wrn_act"    # block output -> (the BN it was activated with, relu(bn(output))) of the fused eval chain


def _take_act(x, bn):
    """The activation the producing block stored for `bn`, if any; the attribute is dropped once read, so a stored block output
    (a hint) does not keep it alive."""
    a = getattr(x, _ACT, None)
    if a is None:
        return None
    delattr(x, _ACT)
    return a[1] if a[0] is bn else None


class BasicBlock(nn.Module):
    def __init__(self, in_planes, out_planes, stride, dropRate=0.0):
        super().__init__()
        self.bn1 = BatchNorm2dNHWC(in_planes)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = Conv2dNHWC(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = BatchNorm2dNHWC(out_planes)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = Conv2dNHWC(out_planes, out_planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.droprate = dropRate
        self.equalInOut = in_planes == out_planes
        self.convShortcut = None if self.equalInOut else Conv2dNHWC(in_planes, out_planes, kernel_size=1, stride=stride,
                                                                    padding=0, bias=False)
        self._next = (None,)     # the BN that reads this block's output (WideResNet sets it; a tuple, not a child module)

    def _fusable(self, x):
        return (x.is_cuda and not self.training and not torch.is_grad_enabled()
                and type(self.conv1) is nn_hip.Conv2dNHWC and type(self.conv2) is nn_hip.Conv2dNHWC
                and type(self.bn1) is nn_hip.BatchNorm2dNHWC and type(self.bn2) is nn_hip.BatchNorm2dNHWC
                and (self.convShortcut is None or type(self.convShortcut) is nn_hip.Conv2dNHWC))

    def _forward_fused(self, x):
        a = _take_act(x, self.bn1)
        if a is None:
            a = self.bn1(x, relu=True)
        ah = self.conv1._input(a)
        if self.equalInOut:
            sc = _nhwc(x)
        else:
            self.convShortcut._check()
            sc = self.convShortcut._run(ah)
        self.conv1._check()
        self.conv2._check()
        s2, b2 = self.bn2.folded()
        _, h = self.conv1._run(ah, out_act=True, act_scale=s2, act_shift=b2, act_relu=True, want_raw=False)
        h = self.conv2._input(nn_hip.mark_padded(h.permute(0, 3, 1, 2)))     # (the view itself; bf16: widened to its zero channels)
        nxt = self._next[0]
        if nxt is None or type(nxt) is not nn_hip.BatchNorm2dNHWC:
            return self.conv2._run(h, res_pre=sc).permute(0, 3, 1, 2)
        s, b = nxt.folded()
        raw, act = self.conv2._run(h, res_pre=sc, out_act=True, act_scale=s, act_shift=b, act_relu=True)
        out = raw.permute(0, 3, 1, 2)
        setattr(out, _ACT, (nxt, nn_hip.mark_padded(act.permute(0, 3, 1, 2))))
        return out

    def forward(self, x):
        drop = self.droprate > 0 and self.training
        if drop and not x.is_cuda:
            raise NotImplementedError("WideResNet: dropout (dropRate > 0) in training runs on the device only (nn_hip.dropout)")
        if self._fusable(x):
            return self._forward_fused(x)
        if not self.equalInOut:
            x = self.bn1(x, relu=True)       # the reference's quirk: conv1 AND the shortcut read relu1(bn1(x))
            out = x
        elif type(self.bn1) is nn_hip.BatchNorm2dNHWC:
            out, x = self.bn1.forward_with_shortcut(x, relu=True)   # the shortcut's gradient joins bn1's dx in its kernel
        else:
            out = self.bn1(x, relu=True)
        out = self.bn2(self.conv1(out), relu=True)
        if drop:        # out of place (bn2 saved its output for its backward), into a padded buffer conv2 reads in place
            out = nn_hip.dropout(out, self.droprate, True)
        sc = x if self.equalInOut else self.convShortcut(x)
        if isinstance(self.conv2, nn_hip.Conv2dNHWC):
            return self.conv2(out, residual=sc)
        return torch.add(sc, self.conv2(out))


class NetworkBlock(nn.Module):
    def __init__(self, nb_layers, in_planes, out_planes, block, stride, dropRate=0.0):
        super().__init__()
        self.layer = nn.Sequential(*[block(in_planes if i == 0 else out_planes, out_planes, stride if i == 0 else 1, dropRate)
                                     for i in range(nb_layers)])

    def forward(self, x):
        return self.layer(x)


class WideResNet(nn.Module):
    def __init__(self, depth, num_classes, widen_factor=1, dropRate=0.0):
        super().__init__()
        nch = [16, 16 * widen_factor, 32 * widen_factor, 64 * widen_factor]
        assert (depth - 4) % 6 == 0, "depth should be 6n+4"
        n = (depth - 4) // 6
        self.conv1 = Conv2dNHWC(3, nch[0], kernel_size=3, stride=1, padding=1, bias=False)
        self.block1 = NetworkBlock(n, nch[0], nch[1], BasicBlock, 1, dropRate)
        self.block2 = NetworkBlock(n, nch[1], nch[2], BasicBlock, 2, dropRate)
        self.block3 = NetworkBlock(n, nch[2], nch[3], BasicBlock, 2, dropRate)
        self.bn1 = BatchNorm2dNHWC(nch[3])
        self.relu = nn.ReLU(inplace=True)
        self.fc = nn.Linear(nch[3], num_classes)
        self.nChannels = nch[3]
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / fan))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                m.bias.data.zero_()
        blocks = [b for g in (self.block1, self.block2, self.block3) for b in g.layer]
        for b, nxt in zip(blocks, [b.bn1 for b in blocks[1:]] + [self.bn1]):
            b._next = (nxt,)

    def forward(self, x):
        out = self.conv1(x)
        out = self.block3(self.block2(self.block1(out)))
        a = _take_act(out, self.bn1) if out.is_cuda and not self.training and not torch.is_grad_enabled() else None
        if a is None:
            a = self.bn1(out, relu=True)
        out = F.avg_pool2d(a.float(), 8)      # (bf16 activations end here: pool, fc and the logits are fp32)
        return self.fc(out.reshape(-1, self.nChannels))


def wrn(**kwargs):
    """Constructs a Wide Residual Network (depth, num_classes, widen_factor, dropRate)."""
    return WideResNet(**kwargs)
