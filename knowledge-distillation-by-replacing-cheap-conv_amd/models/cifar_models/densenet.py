"""CIFAR DenseNet-BC (Huang et al.; DenseNet-121 is the teacher of cfg/cifar10/densenet121/config1-5.json) with the reference's
module tree and state-dict keys (models/cifar_models/densenet.py): features.{conv0, norm0, relu0, pool0},
features.denseblockK.denselayerJ.{norm1, relu1, conv1, norm2, relu2, conv2}, features.transitionK.{norm, relu, conv, pool},
features.norm5, classifier -- so a checkpoint loads through forgiving_state_restore and every block name of the configs
resolves.  Same constructors and initialisation rule.

Channels-last fp32 throughout, as in wrn.py: convolutions are nn_hip.Conv2dNHWC, BatchNorm nn_hip.BatchNorm2dNHWC, the stem's
max pool and the transitions' average pool nn_hip.MaxPool3x3s2NHWC / AvgPool2x2NHWC.  The final ReLU, the 1x1 average pool and
`classifier` are torch ops.

A dense block runs without a concatenation.  Its forward allocates ONE (N,H,W,C_end) NHWC buffer, copies the block input into
channels [0:C0], and every layer's conv2 writes its growth_rate channels straight into its slice (a replaced conv2 -- a
DepthwiseSeparableBlock -- is copied in with one kd_copy_cast).  A layer's output is the NCHW-logical view of the prefix
[0 : C_in + growth] of that storage: hooks on denselayerJ / denseblockK see values equal to the reference's torch.cat, a hook
on conv2 sees the 32-channel slice.

Train mode: the batch statistics of a channel of the buffer are the same for every later norm1, so they are reduced once per
slice (kd_bn_nhwc_stats) and each norm1 -- and the transition's norm / norm5 that read the whole block -- is one
kd_bn_nhwc_apply pass.  They live for the block's forward (and in the autograd graph as the saved statistics).  Backward: the
layers form a chain, norm1's backward adds the gradient of the prefix it read (kd_bn_nhwc_bwd's `res`) and accumulates in place
into the buffer the next layer's norm1 allocated (nn_hip.GradChain), so the block's input gradients live in one buffer too.

drop_rate > 0 in train mode: conv2 writes a temporary and one kd_dropout_nhwc pass (nn_hip.dropout, out= the layer's slice) moves
the dropped features into the buffer, in place of the copy; the slice's statistics are reduced from the dropped values, and the
backward is the same pass over the slice of the gradient (the mask is regenerated from the call's (seed, offset), not stored).

Eval mode without autograd (the frozen teacher, validation): conv1's epilogue applies norm2 + ReLU folded to scale / shift, while
both convs and both BNs of the layer are the nn_hip classes and conv1 / norm2 / relu2 carry no hooks.  norm1 and conv2 are
called as modules either way (the configs hint conv2).

Host tensors (nn_hip.allow_host_tensors) run the torch base classes and torch.cat, like the reference.
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import nn_hip, ops
from ...nn_hip import AvgPool2x2NHWC, BatchNorm2dNHWC, Conv2dNHWC, GradChain, MaxPool3x3s2NHWC, _copy_cast, _hooked

__all__ = ["DenseNet", "densenet121", "densenet169", "densenet201", "densenet161"]

_STATS = "_densenet_stats"    # block output -> (eps, mean, invstd, var_unbiased) of its channels, for the BN that reads it next


def _take_stats(x, bn):
    """The batch statistics the producing block left on `x`, if `bn` can use them; dropped once read (a stored hint stays light)."""
    st = getattr(x, _STATS, None)
    if st is None:
        return None
    delattr(x, _STATS)
    if not bn.training or st[0] != bn.eps or st[1].numel() != bn.num_features:
        return None
    return st[1:]


class _BlockState:
    """One forward of a dense block: the shared buffer, the per-channel batch statistics (train mode) and the backward's chain."""

    def __init__(self, x, c_end, want_stats, eps):
        N, _, H, W = x.shape
        self.buf = torch.empty((N, H, W, c_end), dtype=torch.float32, device=x.device)
        self.eps = eps
        self.stat = [torch.empty(c_end, device=x.device) for _ in range(3)] if want_stats else None
        self.chain = GradChain()

    def view(self, c0, c1):
        """NCHW-logical view of channels [c0:c1] of the buffer."""
        return self.buf[..., c0:c1].permute(0, 3, 1, 2)

    def produced(self, c0, c1):
        if self.stat is not None:
            ops.bn_nhwc_stats(self.buf[..., c0:c1], self.eps, *(v[c0:c1] for v in self.stat))

    def stats_for(self, bn, c):
        if self.stat is None or not bn.training or bn.eps != self.eps:
            return None
        return tuple(v[:c] for v in self.stat)


class _EnterFn(torch.autograd.Function):
    """The block input copied into channels [0:C0] of the buffer -> that prefix view."""

    @staticmethod
    def forward(ctx, x, st):
        c0 = x.shape[1]
        _copy_cast(x, st.view(0, c0))
        return st.view(0, c0)

    @staticmethod
    def backward(ctx, gy):
        return gy, None


class _AppendFn(torch.autograd.Function):
    """(prefix [0:c_in], the layer's new features) -> prefix [0 : c_in + growth] of the same storage.  conv2 has already written
    its slice (copy=False) or `new` is copied in.  Backward: the two channel ranges of the gradient, as views."""

    @staticmethod
    def forward(ctx, xs, new, st, c_in, copy):
        ctx.c_in = c_in
        c1 = c_in + new.shape[1]
        if copy:
            _copy_cast(new, st.view(c_in, c1))
        return st.view(0, c1)

    @staticmethod
    def backward(ctx, gy):
        return gy[:, :ctx.c_in], gy[:, ctx.c_in:], None, None, None


class _DenseLayer(nn.Sequential):
    def __init__(self, num_input_features, growth_rate, bn_size, drop_rate):
        super().__init__()
        self.add_module("norm1", BatchNorm2dNHWC(num_input_features))
        self.add_module("relu1", nn.ReLU(inplace=True))
        self.add_module("conv1", Conv2dNHWC(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, bias=False))
        self.add_module("norm2", BatchNorm2dNHWC(bn_size * growth_rate))
        self.add_module("relu2", nn.ReLU(inplace=True))
        self.add_module("conv2", Conv2dNHWC(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False))
        self.drop_rate = drop_rate
        self.num_input_features = num_input_features
        self.growth_rate = growth_rate

    def _fusable(self, x):
        return (not self.training and not torch.is_grad_enabled()
                and type(self.conv1) is nn_hip.Conv2dNHWC and type(self.conv2) is nn_hip.Conv2dNHWC
                and type(self.norm1) is nn_hip.BatchNorm2dNHWC and type(self.norm2) is nn_hip.BatchNorm2dNHWC
                and not self.norm2.training and not _hooked(self.conv1, self.norm2, self.relu2))

    def forward(self, x, st=None):
        drop = self.drop_rate > 0 and self.training
        if drop and not x.is_cuda:
            raise NotImplementedError("DenseNet: dropout (drop_rate > 0) in training runs on the device only (nn_hip.dropout)")
        if nn_hip._host(x):
            return torch.cat([x, super().forward(x)], 1)
        c_in, c1 = self.num_input_features, self.num_input_features + self.growth_rate
        if x.shape[1] != c_in:
            raise ValueError(f"_DenseLayer: {x.shape[1]} input channels, built for {c_in}")
        if st is None:                       # a layer called on its own: a block of one
            st = _BlockState(x, c1, self.training, self.norm1.eps)
            x = _EnterFn.apply(x, st)
            st.produced(0, c_in)
        into = st.buf[..., c_in:c1]
        if self._fusable(x):
            a = self.norm1(x, relu=True)
            self.conv1._check()
            s2, b2 = self.norm2.folded()
            _, h = self.conv1._run(self.conv1._input(a), out_act=True, act_scale=s2, act_shift=b2, act_relu=True, want_raw=False)
            xs, new, copy = x, self.conv2(h.permute(0, 3, 1, 2), out=into), False
        else:
            if type(self.norm1) is nn_hip.BatchNorm2dNHWC:   # the prefix's gradient joins norm1's dx in its kernel
                a, xs = self.norm1.forward_with_stats(x, st.stats_for(self.norm1, c_in), relu=True, shortcut=True, chain=st.chain)
            else:
                a, xs = self.relu1(self.norm1(x)), x
            h = self.conv1(a)
            h = self.norm2(h, relu=True) if isinstance(self.norm2, nn_hip.BatchNorm2dNHWC) else self.relu2(self.norm2(h))
            if drop:    # conv2 writes a temporary (what a hook on it sees, as in the reference); the dropout pass moves it into the slice
                new, copy = nn_hip.dropout(self.conv2(h), self.drop_rate, True, out=into), False
            elif type(self.conv2) is nn_hip.Conv2dNHWC:
                new, copy = self.conv2(h, out=into), False
            else:
                new, copy = self.conv2(h), True
        out = _AppendFn.apply(xs, new, st, c_in, copy)
        st.produced(c_in, c1)
        return out


class _DenseBlock(nn.Sequential):
    def __init__(self, num_layers, num_input_features, bn_size, growth_rate, drop_rate):
        super().__init__()
        for i in range(num_layers):
            self.add_module("denselayer%d" % (i + 1), _DenseLayer(num_input_features + i * growth_rate, growth_rate, bn_size, drop_rate))
        self.num_input_features = num_input_features
        self.num_output_features = num_input_features + num_layers * growth_rate

    def forward(self, x):
        if nn_hip._host(x):
            return super().forward(x)
        if x.dtype != torch.float32:
            raise TypeError("DenseNet is fp32 (the CIFAR path of the reference is fp32)")
        layers = list(self.children())
        eps = layers[0].norm1.eps
        st = _BlockState(x, self.num_output_features, self.training, eps)
        out = _EnterFn.apply(x, st)
        st.produced(0, self.num_input_features)
        for layer in layers:
            out = layer(out, st)
        if st.stat is not None:
            setattr(out, _STATS, (eps, *st.stat))
        return out


def _bn_relu(bn, relu, x):
    if isinstance(bn, nn_hip.BatchNorm2dNHWC):
        return bn(x, relu=True, stats=_take_stats(x, bn))
    return relu(bn(x))


class _Transition(nn.Sequential):
    def __init__(self, num_input_features, num_output_features):
        super().__init__()
        self.add_module("norm", BatchNorm2dNHWC(num_input_features))
        self.add_module("relu", nn.ReLU(inplace=True))
        self.add_module("conv", Conv2dNHWC(num_input_features, num_output_features, kernel_size=1, stride=1, bias=False))
        self.add_module("pool", AvgPool2x2NHWC(kernel_size=2, stride=2))

    def forward(self, x):
        if nn_hip._host(x):
            return super().forward(x)
        return self.pool(self.conv(_bn_relu(self.norm, self.relu, x)))    # (conv, then pool: a hook on conv sees full resolution)


class _Features(nn.Sequential):
    def forward(self, x):
        if nn_hip._host(x):
            return super().forward(x)
        mods = list(self.children())
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.BatchNorm2d) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU):
                x = _bn_relu(m, mods[i + 1], x)          # norm0 + relu0 in one kernel
                i += 2
                continue
            x = m(x, stats=_take_stats(x, m)) if isinstance(m, nn_hip.BatchNorm2dNHWC) else m(x)
            i += 1
        return x


class DenseNet(nn.Module):
    """DenseNet-BC: growth_rate filters per layer, block_config layers per block, num_init_features stem filters,
    bn_size * growth_rate bottleneck width, drop_rate on each layer's new features in train mode (nn_hip.dropout, device tensors
    only: the pass that moves conv2's output into the block buffer), num_classes."""

    def __init__(self, growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4, drop_rate=0, num_classes=10):
        super().__init__()
        # the CIFAR stem: 3x3 / stride 1 (not ImageNet's 7x7 / stride 2)
        self.features = _Features(OrderedDict([
            ("conv0", Conv2dNHWC(3, num_init_features, kernel_size=3, stride=1, padding=1, bias=False)),
            ("norm0", BatchNorm2dNHWC(num_init_features)),
            ("relu0", nn.ReLU(inplace=True)),
            ("pool0", MaxPool3x3s2NHWC(kernel_size=3, stride=2, padding=1)),
        ]))
        num_features = num_init_features
        for i, num_layers in enumerate(block_config):
            self.features.add_module("denseblock%d" % (i + 1), _DenseBlock(num_layers, num_features, bn_size, growth_rate, drop_rate))
            num_features += num_layers * growth_rate
            if i != len(block_config) - 1:
                self.features.add_module("transition%d" % (i + 1), _Transition(num_features, num_features // 2))
                num_features //= 2
        self.features.add_module("norm5", BatchNorm2dNHWC(num_features))
        self.classifier = nn.Linear(num_features, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        features = self.features(x)
        out = F.relu(features)
        out = F.adaptive_avg_pool2d(out, (1, 1)).flatten(1)
        return self.classifier(out)


def _densenet(arch, growth_rate, block_config, num_init_features, pretrained, progress, device, **kwargs):
    if pretrained:
        raise NotImplementedError(f"{arch}(pretrained=True): no state dicts are shipped with this package; build the model and "
                                  "load a checkpoint (the config's `snapshot`) instead")
    return DenseNet(growth_rate, block_config, num_init_features, **kwargs)


def densenet121(pretrained=False, progress=True, device="cpu", **kwargs):
    """DenseNet-121: growth 32, blocks (6, 12, 24, 16), 64 stem filters."""
    return _densenet("densenet121", 32, (6, 12, 24, 16), 64, pretrained, progress, device, **kwargs)


def densenet161(pretrained=False, progress=True, device="cpu", **kwargs):
    """DenseNet-161: growth 48, blocks (6, 12, 36, 24), 96 stem filters."""
    return _densenet("densenet161", 48, (6, 12, 36, 24), 96, pretrained, progress, device, **kwargs)


def densenet169(pretrained=False, progress=True, device="cpu", **kwargs):
    """DenseNet-169: growth 32, blocks (6, 12, 32, 32), 64 stem filters."""
    return _densenet("densenet169", 32, (6, 12, 32, 32), 64, pretrained, progress, device, **kwargs)


def densenet201(pretrained=False, progress=True, device="cpu", **kwargs):
    """DenseNet-201: growth 32, blocks (6, 12, 48, 32), 64 stem filters."""
    return _densenet("densenet201", 32, (6, 12, 48, 32), 64, pretrained, progress, device, **kwargs)
