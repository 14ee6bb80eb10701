"""Stock-torch float64 Wide-ResNet forward and backward that rounds to bf16 where the bf16 module path rounds (CPU).

`R` rounds its value to bf16 (nearest-even) forward and the gradient backward: placed on a tensor the kernels store in bf16, it
stands for the store of the value and for the store of its gradient.  The rounding points of models/cifar_models/wrn.py on
nn_hip.Conv2dNHWC / BatchNorm2dNHWC in bf16:
  * the batch, once;
  * a conv reads bf16 activations and bf16-packed weights (the fp32 master weight gets the gradient unrounded, in fp32), accumulates
    in fp32, adds the residual in its epilogue and stores once: R(conv(a, q(w)) + res).  The R of a stored tensor rounds, backward,
    the sum of what its readers send: a conv's input gradient, stored in bf16; a BatchNorm's; where a block keeps its width, the
    identity shortcut's gradient and bn1's input gradient, which the kernel adds before its one store.  The residual's gradient is
    the output gradient itself;
  * a BatchNorm reads bf16, takes its statistics in fp32 / fp64, and stores relu(bn(x)) once: R(relu(bn(.)));
  * where the width changes, conv1 and the shortcut conv both read the activation: each stores its own bf16 input gradient (an R
    per reader) and autograd adds the two in bf16 (the activation's R);
  * a cheap-conv block stores the depthwise output and the pointwise output in bf16, with fp32 depthwise taps and bf16-packed
    pointwise weights, and the block adds the shortcut to it with a bf16 torch.add: three stores;
  * the last bn1 + ReLU output is widened to fp32: pool, fc, logits and the criteria are not rounded; parameter gradients and running
    statistics are fp32 results of bf16 operands and are not rounded either;
  * the fused eval path (no autograd) stores fewer tensors: conv1's epilogue applies bn2 + ReLU to the fp32 accumulator, conv2's
    stores the block output and, from the same accumulator, the next BatchNorm + ReLU of it (forward_fused).
With emulate=False every R and q is the identity: the exact float64 network (tests/_wrnref.wrn_forward's, plus the cheap-conv
blocks and the hints)."""
import torch
import torch.nn.functional as F


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def bf16(t):
    """Value of t after a nearest-even rounding to bf16, in t's dtype (no autograd)."""
    return t.detach().to(torch.bfloat16).to(t.dtype)


class Net:
    """forward(sd, x) over a state dict of float64 tensors (those that require grad receive their gradients).
    cheap: {conv name: (depthwise weight, pointwise weight)} for convs replaced by a cheap-conv block (3x3, padding 1).
    hints: block names ("block3.layer.0", "block3") whose outputs are returned in `self.hints`, in forward order."""

    def __init__(self, depth, emulate=True, cheap=None, hints=()):
        self.n = (depth - 4) // 6
        self.emulate = emulate
        self.cheap = cheap or {}
        self.hint_names = tuple(hints)
        self.hints = []

    def R(self, t):
        return _Round.apply(t) if self.emulate else t

    def q(self, w):
        """The bf16-packed copy of an fp32 master weight: rounded value, gradient straight through."""
        return w + (bf16(w) - w.detach()) if self.emulate else w

    def bn(self, sd, p, x, training):
        return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], training, 0.1, 1e-5)

    def conv(self, sd, name, a, stride=1, padding=1, res=None):
        """a: an activation that carries its R (the R also stores this conv's input gradient).  The output's R rounds the value
        once and, backward, the sum of the gradients its readers send."""
        if name in self.cheap:      # two stores, and the residual is added by a bf16 torch.add afterwards: a third
            wdw, wpw = self.cheap[name]
            mid = self.R(F.conv2d(a, wdw, padding=1, groups=a.shape[1]))
            y = self.R(F.conv2d(mid, self.q(wpw)))
        else:
            y = F.conv2d(a, self.q(sd[name + ".weight"]), stride=stride, padding=padding)
        return self.R(y if res is None else y + res)

    def forward(self, sd, x, training=False):
        R = self.R
        self.hints = []
        out = self.conv(sd, "conv1", R(x))
        for g in (1, 2, 3):
            for i in range(self.n):
                p = f"block{g}.layer.{i}"
                stride = 2 if (g > 1 and i == 0) else 1
                a = R(F.relu(self.bn(sd, p + ".bn1", out, training)))
                if (p + ".convShortcut.weight") in sd:
                    a1 = R(a)                                 # each of the two convs stores its own bf16 input gradient ...
                    sc = self.conv(sd, p + ".convShortcut", R(a), stride, 0)      # ... and a's R adds them in bf16
                else:
                    a1, sc = a, out                           # out's R: shortcut gradient + bn1's input gradient, one store
                h = self.conv(sd, p + ".conv1", a1, stride)
                h = R(F.relu(self.bn(sd, p + ".bn2", h, training)))
                out = self.conv(sd, p + ".conv2", h, res=sc)
                if p in self.hint_names:
                    self.hints.append(out)
            if f"block{g}" in self.hint_names:
                self.hints.append(out)
        out = R(F.relu(self.bn(sd, "bn1", out, training)))
        out = F.adaptive_avg_pool2d(out, 1).flatten(1)
        return F.linear(out, sd["fc.weight"], sd["fc.bias"])


    @torch.no_grad()
    def forward_fused(self, sd, x):
        """Eval-mode logits by the rounding points of the fused chain (plain convs only)."""
        R = self.R
        conv = lambda name, a, stride=1, padding=1: F.conv2d(a, bf16(sd[name + ".weight"]) if self.emulate else sd[name + ".weight"], stride=stride,
                                                             padding=padding)
        self.hints = []
        out = R(conv("conv1", R(x)))
        a = None
        for g in (1, 2, 3):
            for i in range(self.n):
                p = f"block{g}.layer.{i}"
                stride = 2 if (g > 1 and i == 0) else 1
                if a is None:
                    a = R(F.relu(self.bn(sd, p + ".bn1", out, False)))
                sc = R(conv(p + ".convShortcut", a, stride, 0)) if (p + ".convShortcut.weight") in sd else out
                h = R(F.relu(self.bn(sd, p + ".bn2", conv(p + ".conv1", a, stride), False)))
                raw = conv(p + ".conv2", h) + sc
                nxt = f"block{g}.layer.{i + 1}.bn1" if i + 1 < self.n else (f"block{g + 1}.layer.0.bn1" if g < 3 else "bn1")
                out, a = R(raw), R(F.relu(self.bn(sd, nxt, raw, False)))
                if p in self.hint_names:
                    self.hints.append(out)
            if f"block{g}" in self.hint_names:
                self.hints.append(out)
        return F.linear(F.adaptive_avg_pool2d(a, 1).flatten(1), sd["fc.weight"], sd["fc.bias"])


def kld(s, t, T):
    """losses.KLDivergenceLoss: kl_div(log_softmax(s / T), softmax(t / T), 'mean') * T^2 * C"""
    return F.kl_div(F.log_softmax(s / T, 1), F.softmax(t / T, 1), reduction="mean") * T * T * s.shape[1]


def double_sd(module, trainable=lambda name: True):
    """float64 copies of a module's state dict; parameters `trainable` names require grad."""
    params = {n for n, _ in module.named_parameters()}
    return {k: v.detach().clone().double().requires_grad_(k in params and trainable(k)) for k, v in module.state_dict().items()
            if v.is_floating_point()}
