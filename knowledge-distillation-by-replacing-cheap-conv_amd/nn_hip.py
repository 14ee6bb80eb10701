"""nn.Conv2d / nn.BatchNorm2d whose forward and backward run on the small-shape HIP kernels (include/kdcc.h,
kd_conv2d_direct_*, kd_bn2d_*) when the tensors live on the GPU.  Same constructors, parameters, buffers and state-dict
keys as the torch classes, so checkpoints, forward hooks (hint layers) and DepthwiseStudent's module surgery are untouched.
Used by the CIFAR plumbing config (models/cifar_models): with them a ClassificationTrainer step issues no MIOpen kernel.

There is no silent fallback: a device tensor either goes through the kernels or raises, and a HOST tensor raises too unless
host plumbing mode was switched on explicitly (`allow_host_tensors(True)`: BaseTrainer does it for `n_gpu: 0` configs -- the
reference's CPU plumbing case, BASELINE config 1 -- and the CPU-only host-logic tests do it themselves).  In that mode the
modules behave exactly like their torch base classes; it is never the measured or parity-tested path.
"""
import copy

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from ._lib import KD_PACK_DGRAD, KD_PACK_FWD, KdccError

_HOST_OK = False


def allow_host_tensors(on=True):
    """Host plumbing mode (n_gpu = 0): Conv2d / BatchNorm2d given host tensors run their torch base class.  Off by default."""
    global _HOST_OK
    _HOST_OK = bool(on)


def _host(x):
    if x.is_cuda:
        return False
    if not _HOST_OK:
        raise KdccError("kdcc nn_hip modules got a host tensor: the HIP kernels need device tensors and there is no silent CPU "
                        "fallback (host plumbing runs, `n_gpu: 0`, call nn_hip.allow_host_tensors(True) -- BaseTrainer does)")
    return True


def _one(v):
    """A square geometry argument (an int, or a pair of equal ints) as one int; anything else comes back as given."""
    return v[0] if isinstance(v, (tuple, list)) and len({*v}) == 1 else v


def _hooked(*mods):
    return any(m._forward_hooks or m._forward_pre_hooks for m in mods)


def _deepcopy_without(mod, memo, **fresh):
    """copy.deepcopy(mod) that does not carry the cached device tensors over: the attributes named in `fresh` start from the
    values given there."""
    new = mod.__class__.__new__(mod.__class__)
    memo[id(mod)] = new
    new.__dict__.update({k: copy.deepcopy(v, memo) for k, v in mod.__dict__.items() if k not in fresh})
    new.__dict__.update(fresh)
    return new


class _DirectConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil, groups):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w)
        ctx.geom = (stride, pad, dil, groups, bias is not None)
        return ops.conv2d_direct(x, w, None if bias is None else bias.contiguous(), stride, pad, dil, groups)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, pad, dil, groups, has_bias = ctx.geom
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = ops.conv2d_direct_dgrad(gy, w, x.shape, stride, pad, dil, groups)
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            gw, gb = ops.conv2d_direct_wgrad(x, gy, w.shape, stride, pad, dil, groups, want_bias=has_bias)
        return gx, gw, gb, None, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    """F.conv2d on the direct HIP kernels (device fp32 NCHW) / torch (host tensors)."""
    if _host(x):
        return F.conv2d(x, weight, bias, stride, padding, dilation, groups)
    if x.dtype != torch.float32:
        raise TypeError("the small-shape conv kernels are fp32 (the CIFAR path of the reference is fp32)")
    return _DirectConv.apply(x, weight, bias, _one(stride), _one(padding), _one(dilation), groups)


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, relu):
        x = x.contiguous()
        y, mean, invstd = ops.bn2d_fwd(x, gamma.contiguous(), beta.contiguous(), running_mean, running_var, training, momentum, eps, relu)
        ctx.save_for_backward(x, y if relu else x, gamma, mean, invstd)
        ctx.flags = (training, relu)
        ctx.mark_non_differentiable(mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, gamma, mean, invstd = ctx.saved_tensors
        training, relu = ctx.flags
        dx, dg, db = ops.bn2d_bwd(gy.contiguous(), x, y, gamma.contiguous(), mean, invstd, training, relu,
                                  need_dx=ctx.needs_input_grad[0])
        return dx, dg if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None, None, None, None, None, None


class Conv2d(nn.Conv2d):
    def forward(self, x):
        if _host(x):
            return super().forward(x)
        if self.padding_mode != "zeros" or isinstance(self.padding, str) or len({*self.stride}) != 1 or len({*self.padding}) != 1 \
                or len({*self.dilation}) != 1:
            raise NotImplementedError("HIP Conv2d: square zero-padded geometry only")
        return conv2d(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups)


class BatchNorm2d(nn.BatchNorm2d):
    def forward(self, x, relu=False):
        if _host(x):
            y = super().forward(x)
            return F.relu(y) if relu else y
        if not (self.affine and self.track_running_stats) or self.momentum is None:
            raise NotImplementedError("HIP BatchNorm2d: affine, running statistics, fixed momentum")
        if x.dtype != torch.float32:
            raise TypeError("HIP BatchNorm2d is fp32")
        if self.training:
            self.num_batches_tracked.add_(1)
        return _BatchNorm.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.training, float(self.momentum),
                                float(self.eps), bool(relu))


# ------------------------------------------------------------------ channels-last modules (Wide-ResNet, DenseNet, HRNet-OCR)
# NCHW-logical tensors with NHWC strides (torch.channels_last): the MFMA implicit-GEMM convolutions (kd_conv2d_fwd /
# kd_conv2d_wgrad / kd_pw_wgrad) and BatchNorm on NHWC views (kd_bn_nhwc_*) read and write them without a layout copy.  fp32
# everywhere; Conv2dNHWC and BatchNorm2dNHWC also take bf16 activations (fp32 parameters and parameter gradients).
_CIN_GRANULE = 32      # fp32 K granule of kd_conv2d_fwd: fewer input channels are zero-padded up to it (the 3->16 stem, 16->160)
_GRANULE = {torch.float32: _CIN_GRANULE, torch.bfloat16: 64}   # ... per activation dtype: kd_conv2d_fwd takes Cin % 64 in bf16
_PADDED = "_nhwc_pad"  # tensor attribute: its NHWC storage continues with zero channels up to this pixel stride


def _granule_up(c, dtype=torch.float32):
    g = _GRANULE[dtype]
    return -(-c // g) * g


def _copy_cast(src, dst):
    """dst = src for two (N,C,H,W)-logical tensors of any dense-plane layout: one kd_copy_cast."""
    try:
        ops.copy_cast(src, dst)
    except ValueError:              # (rows that are not one plane: make them so first)
        ops.copy_cast(src.contiguous(), dst)


def _copy_into(src, dst):
    """dst = src for two (N,H,W,C) views (dst a channel slice of a wider buffer)."""
    _copy_cast(src.permute(0, 3, 1, 2), dst.permute(0, 3, 1, 2))


def _nhwc(t):
    """(N,C,H,W)-logical tensor -> (N,H,W,C) view; a kd_copy_cast copy only when t is not channels_last-strided."""
    v = t.permute(0, 2, 3, 1)
    try:
        ops.nhwc_ld(v)
        if v.data_ptr() % 16 == 0 and (v.stride(2) * v.element_size()) % 16 == 0:
            return v
    except ValueError:
        pass
    N, Cc, H, W = t.shape
    out = torch.empty((N, H, W, Cc), dtype=t.dtype, device=t.device)
    _copy_cast(t, out.permute(0, 3, 1, 2))
    return out


def _nhwc_padded(t, cpad):
    """(N,C,H,W)-logical tensor -> (N,H,W,cpad) buffer of its dtype, channels >= C zero (the conv's K granule): a padding copy."""
    N, Cc, H, W = t.shape
    out = torch.zeros((N, H, W, cpad), dtype=t.dtype, device=t.device)
    _copy_cast(t, out[..., :Cc].permute(0, 3, 1, 2))
    return out


def new_padded(shape, device, dtype=torch.float32):
    """(N,H,W,C) view for a kernel to fill.  When C is no multiple of the dtype's conv granule the view is the channel prefix of a
    buffer whose pixel stride is the granule above C, with a zero tail: tagged with mark_padded(), a conv reads it in place."""
    N, H, W, Cc = shape
    buf = torch.empty((N, H, W, _granule_up(Cc, dtype)), dtype=dtype, device=device)
    if buf.shape[3] != Cc:
        buf[..., Cc:].zero_()
    return buf[..., :Cc]


def mark_padded(t):
    """Tag an NCHW-logical tensor whose storage came from new_padded() (and was written through its view only)."""
    v = t.permute(0, 2, 3, 1)
    cpad = _granule_up(v.shape[3], t.dtype)
    if cpad != v.shape[3] and v.stride(3) == 1 and v.stride(2) == cpad:
        setattr(t, _PADDED, cpad)
    return t


class _ConvNHWCFn(torch.autograd.Function):
    """xh: the module's input view (Conv2dNHWC._input of x), made by the caller, where x still carries its padding tag."""

    @staticmethod
    def forward(ctx, x, weight, bias, res, mod, xh, out):
        y = mod._run(xh, res_pre=None if res is None else _nhwc(res), raw_into=out)
        ctx.mod = mod
        ctx.in_shape = tuple(x.shape)
        ctx.save_for_backward(xh if weight.requires_grad else None)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        mod = ctx.mod
        (xh,) = ctx.saved_tensors
        co, cop = mod.out_channels, mod._cout_pad(gy.dtype, dgrad=ctx.needs_input_grad[0])
        g = _nhwc(gy) if co == cop else _nhwc_padded(gy, cop)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = mod._dgrad(g, ctx.in_shape).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            dw = mod._wgrad(xh, g)
        if ctx.needs_input_grad[2]:       # the bias gradient is a channel sum, taken only when somebody wants it
            db = ops.channel_sums(g)[0][:co]
        return dx, dw, db, gy if ctx.needs_input_grad[3] else None, None, None, None


class Conv2dNHWC(nn.Conv2d):
    """nn.Conv2d (3x3 or 1x1, square stride / padding, no groups, optional bias) on channels-last fp32 or bf16 device tensors:
    forward kd_conv2d_fwd; input gradient kd_conv2d_fwd on KD_PACK_DGRAD weights (zero-inserted first for stride 2);
    weight gradient kd_conv2d_wgrad / kd_pw_wgrad, computed only for a weight that requires grad; the bias is the forward
    epilogue's per-channel shift (scale 1, no ReLU), its gradient a channel sum taken only when it requires grad.  Packed
    weights (and the shift vector) are cached per parameter version: a frozen one is packed once, a trained one once per
    optimizer step.  Fewer than 32 input channels are zero-padded to 32 (weights packed with cin_pad, the input copied into a
    zeroed 32-channel buffer); an input whose storage is already zero-padded to that granule (tagged by its producer, see
    new_padded() / mark_padded()) is read in place instead.
    bf16 activations (this class only, not Conv2dNHWCBias): the parameters stay fp32 and are packed to bf16 (the cache is keyed by
    dtype as well as mode); outputs, the residual and the input gradient are bf16; bias and fold vectors stay fp32; the weight
    gradient comes back in fp32.  The K granule is 64: an input channel count that is no multiple of it (16 -> 64, 160 -> 192) is
    read from a zero-padded buffer as above, and in the backward the output gradient -- the K operand of the input-gradient conv
    -- is padded likewise (a padding copy: gradients arrive untagged), with the weights packed to match.  The activated output
    of the fused eval path is allocated by new_padded(), so the next conv reads it in place.
    forward(x, residual=None, out=None): residual (the block's shortcut) is added in the conv's epilogue; out, an (N,Ho,Wo,Cout)
    fp32 NHWC view (a channel slice of a wider buffer: a dense block's), receives the result instead of a fresh tensor.
    run_folded() puts an eval-mode BN (+ ReLU) into the epilogue as well.

    pad_channels says what happens to an output channel count that is no multiple of the granule.  Off (this class): outputs
    are dense tensors (or the caller's `out`), the output gradient is used as it arrives, so Cout is what the kernels take.
    On (Conv2dNHWCBias): see there."""

    pad_channels = False

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._packs = {}

    def __deepcopy__(self, memo):
        return _deepcopy_without(self, memo, _packs={})

    def _check(self):
        k, s, p = self.kernel_size, self.stride, self.padding
        if self.padding_mode != "zeros" or isinstance(p, str) or k[0] != k[1] or k[0] not in (1, 3) or s[0] != s[1] or p[0] != p[1] \
                or self.dilation != (1, 1) or self.groups != 1:
            raise NotImplementedError(f"{type(self).__name__}: 1x1 / 3x3, square stride and padding, no dilation or groups")

    def _check_dtype(self, x):
        if x.dtype != torch.float32 and (x.dtype != torch.bfloat16 or self.pad_channels):
            raise TypeError(f"{type(self).__name__} is fp32" + ("" if self.pad_channels else " or bf16"))

    @property
    def cin_pad(self):
        return _granule_up(self.in_channels)

    @property
    def cout_pad(self):
        """Channels of the output gradient the backward works on (and rows of the weights packed for it)."""
        return _granule_up(self.out_channels) if self.pad_channels else self.out_channels

    def _cin_pad(self, dtype):
        return _granule_up(self.in_channels, dtype)

    def _cout_pad(self, dtype, dgrad=False):
        """cout_pad for activations of `dtype`: in bf16 the output gradient is always padded to the K granule of its dgrad conv; in
        fp32 only where that conv runs (dgrad) and needs it: the 16-channel layers of the CIFAR PreResNet."""
        return self.cout_pad if dtype == torch.float32 and not dgrad else _granule_up(self.out_channels, dtype)

    @property
    def cout_fwd(self):
        """Output rows of the forward's packed weight."""
        return self.out_channels if self.out_channels % 16 == 0 else self.cout_pad

    def _padded_rows(self, t, rows=None):
        """Parameter (Cout, ...) -> (rows, ...) with zero rows behind (rows = cout_fwd unless given)."""
        rows = self.cout_fwd if rows is None else rows
        if self.out_channels == rows:
            return t.detach()
        out = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
        out[:self.out_channels].copy_(t.detach())
        return out

    def _cached(self, what, t, make):
        key = (what, t._version, t.data_ptr())
        hit = self._packs.get(what)
        if hit is None or hit[0] != key:
            hit = self._packs[what] = (key, make())
        return hit[1]

    def _pack(self, mode, dtype=torch.float32):
        w = self.weight
        rows, cin_pad = (self.cout_fwd, self._cin_pad(dtype)) if mode == KD_PACK_FWD else (self._cout_pad(dtype, dgrad=True), None)
        what = mode if dtype == torch.float32 else (mode, dtype)
        return self._cached(what, w, lambda: ops.pack_conv_weight(self._padded_rows(w, rows), dtype, mode, cin_pad=cin_pad))

    def _shift(self):
        """The bias as the epilogue's shift vector (cout_fwd long), or None."""
        b = self.bias
        return None if b is None else self._cached("bias", b, lambda: self._padded_rows(b).float().contiguous())

    def _prepadded(self, x):
        """The (N,H,W,cin_pad) view of an input whose producer left zero channels behind it, or None."""
        cin_pad = self._cin_pad(x.dtype)
        if self.in_channels != cin_pad and getattr(x, _PADDED, 0) == cin_pad:
            v = x.detach().permute(0, 2, 3, 1)
            if v.stride(3) == 1 and v.stride(2) == cin_pad:
                N, H, W, _ = v.shape
                return v.as_strided((N, H, W, cin_pad), v.stride())
        return None

    def _input(self, x):
        """The (N,H,W,cin_pad) view the kernels read; called where x still carries its padding tag (not inside a Function)."""
        pre = self._prepadded(x)
        if pre is not None:
            return pre
        if self.in_channels != self._cin_pad(x.dtype):
            return _nhwc_padded(x.detach(), self._cin_pad(x.dtype))
        return _nhwc(x.detach())

    def _run(self, xh, res_pre=None, out_act=False, act_scale=None, act_shift=None, act_relu=False, want_raw=True, raw_into=None,
             act_padded=False):
        """Forward on an (N,H,W,cin_pad) view: raw = conv(xh) + bias [+ res_pre] and, with out_act, act = relu?(act_scale * raw +
        act_shift) -> raw [, act], (N,Ho,Wo,Cout) views of xh's dtype (raw is raw_into when given, None without want_raw).  The
        bias rides in the epilogue's shift, so a biased conv gives raw or act, not both.  In bf16, and in fp32 with act_padded, act
        comes from new_padded()."""
        N, H, W, _ = xh.shape
        k, s, p = self.kernel_size[0], self.stride[0], self.padding[0]
        Ho, Wo = ops.conv_out_size(H, k, s, p, 1), ops.conv_out_size(W, k, s, p, 1)
        co, rows = self.out_channels, self.cout_fwd
        dt = xh.dtype
        if self.pad_channels:
            new = new_act = lambda: new_padded((N, Ho, Wo, rows), xh.device)
        else:
            new = lambda: torch.empty((N, Ho, Wo, co), dtype=dt, device=xh.device)
            new_act = new if dt == torch.float32 and not act_padded else (lambda: new_padded((N, Ho, Wo, co), xh.device, dt))
        raw = raw_into if raw_into is not None else (new() if want_raw else None)
        act = new_act() if out_act else None
        k_raw, k_act, b = raw, act, self._shift()
        if b is not None and out_act:
            if raw is not None:
                raise NotImplementedError(f"{type(self).__name__}: a biased conv gives the raw or the activated output, not both")
            act_shift = act_shift + act_scale * b[:co]
        elif b is not None:                  # the bias alone is the epilogue: the kernel's activated output is conv + bias
            k_raw, k_act, act_shift = None, raw, b
        if act_scale is not None and co != rows:
            act_scale, act_shift = self._padded_rows(act_scale), self._padded_rows(act_shift)
        vec = lambda v: None if v is None else v.contiguous()
        ops.conv2d(xh, self._pack(KD_PACK_FWD, dt), s, p, res_pre=res_pre, out_raw=k_raw, out_act=k_act, act_scale=vec(act_scale),
                   act_shift=vec(act_shift), act_relu=act_relu)
        view = lambda t: t if t is None or co == rows else t[..., :co]
        return (view(raw), view(act)) if out_act else view(raw)

    def run_folded(self, x, bn, relu):
        """relu?(bn(conv(x) + bias)) for an eval-mode BatchNorm2dNHWC in ONE launch (no autograd: frozen layers only)."""
        self._check()
        s, b = bn.folded()
        self._check_dtype(x)
        y = self._run(self._input(x), out_act=True, act_scale=s, act_shift=b, act_relu=relu, want_raw=False)[1].permute(0, 3, 1, 2)
        return mark_padded(y) if self.pad_channels or x.dtype != torch.float32 else y

    def _dgrad(self, g, in_shape):
        N, Cin, H, W = in_shape
        k, s, p = self.kernel_size[0], self.stride[0], self.padding[0]
        if s != 1:
            g = ops.zero_insert(g, s, (H - k + 1 + 2 * p, W - k + 1 + 2 * p))
        dx = torch.empty((N, H, W, Cin), dtype=g.dtype, device=g.device)
        ops.conv2d(g, self._pack(KD_PACK_DGRAD, g.dtype), 1, k - 1 - p, 1, out_raw=dx)
        return dx

    def _wgrad(self, xh, g):
        k, s, p = self.kernel_size[0], self.stride[0], self.padding[0]
        dw = torch.empty((g.shape[3], xh.shape[3], k, k), dtype=torch.float32, device=g.device)
        if k == 1 and s == 1:
            ops.pw_wgrad(xh, g, dw)
        else:
            ops.conv2d_wgrad(xh, g, dw, s, p, 1)
        if dw.shape[0] == self.out_channels and dw.shape[1] == self.in_channels:
            return dw
        return dw[:self.out_channels, :self.in_channels].contiguous()

    def forward(self, x, residual=None, out=None):
        name = type(self).__name__
        if self.pad_channels and (residual is not None or out is not None):
            raise ValueError(f"{name}: no residual / out operands")
        if _host(x):
            if out is not None:
                raise ValueError(f"{name}: out= is a device view")
            y = super().forward(x)
            return y if residual is None else y + residual
        self._check()
        self._check_dtype(x)
        for t in (residual, out):
            if t is not None and t.dtype != x.dtype:
                raise ValueError(f"{name}: residual / out of {t.dtype} next to an input of {x.dtype}")
        y = _ConvNHWCFn.apply(x, self.weight, self.bias, residual, self, self._input(x), out)
        return mark_padded(y) if self.pad_channels else y


class Conv2dNHWCBias(Conv2dNHWC):
    """Conv2dNHWC for any number of output channels (every HRNet layer: the 48-channel branch, the 19 classes of the OCR
    heads).  An output channel count that is no multiple of 16 is computed with the packed weight and bias zero-padded to the
    granule (32 rows for the 19 classes); the output is allocated by new_padded(), returned as a channel view of that buffer and
    tagged by mark_padded(), so that the next conv reads it in place.  In the backward the output gradient is the K operand
    of the input-gradient conv, so there any count that is no multiple of 32 (48) is zero-padded to the granule, with weights
    packed to match; the weight gradient is computed at that many rows and sliced.  No residual / out operands."""

    pad_channels = True


class _BatchNormNHWCFn(torch.autograd.Function):
    """y = relu?(bn(x)); with `shortcut` also returns x itself, whose gradient (the identity shortcut's, when x is a residual block's
    input) is then added to dx by kd_bn_nhwc_bwd's `res` operand instead of by a separate autograd sum.
    stats: (mean, invstd, var_unbiased) of x's channels computed beforehand (ops.bn_nhwc_stats; train mode only): the forward is
    then one kd_bn_nhwc_apply pass and the backward uses them as the saved statistics.
    chain: a GradChain shared by the BNs of one dense block.  The shortcut gradient of such a BN is a channel prefix of the
    gradient buffer the next layer's BN wrote its dx into; when that is what arrives, dx is accumulated into it in place
    (ops.bn_nhwc_bwd(out=res)) and the whole block's input gradients live in one buffer."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, relu, shortcut, stats=None, chain=None):
        ctx.set_materialize_grads(False)
        xh = _nhwc(x)
        if stats is not None and training:
            mean, invstd, var = stats
            y = ops.bn_nhwc_apply(xh, gamma.contiguous(), beta.contiguous(), mean, invstd, var, running_mean, running_var, momentum, relu)
        else:       # y goes where the conv that reads it finds its zero channels (the caller tags it, see mark_padded)
            out = new_padded(tuple(xh.shape), xh.device, x.dtype)
            y, mean, invstd = ops.bn_nhwc_fwd(xh, gamma.contiguous(), beta.contiguous(), running_mean, running_var, training, momentum,
                                              eps, relu, out=out)
        ctx.save_for_backward(xh, y if relu else None, gamma, mean, invstd)
        ctx.flags = (training, relu)
        ctx.chain = chain
        y = y.permute(0, 3, 1, 2)
        return (y, x) if shortcut else y

    @staticmethod
    def backward(ctx, gy, gsc=None):
        xh, y, gamma, mean, invstd = ctx.saved_tensors
        training, relu = ctx.flags
        Cc = xh.shape[3]
        dg = torch.empty(Cc, device=xh.device) if ctx.needs_input_grad[1] else None
        db = torch.empty(Cc, device=xh.device) if ctx.needs_input_grad[2] else None
        res = None if gsc is None or not ctx.needs_input_grad[0] else _nhwc(gsc)
        if gy is None:
            if dg is not None:
                dg.zero_()
            if db is not None:
                db.zero_()
            return None if res is None else gsc, dg, db, None, None, None, None, None, None, None, None, None
        chain = ctx.chain
        into = res if chain is not None and res is not None and chain.owns(res) else None
        dx = ops.bn_nhwc_bwd(_nhwc(gy), xh, y, gamma.contiguous(), mean, invstd, training, relu, res=res,
                             need_dx=ctx.needs_input_grad[0], dgamma=dg, dbeta=db, out=into)
        if chain is not None and dx is not None:
            chain.buf = dx
        return None if dx is None else dx.permute(0, 3, 1, 2), dg, db, None, None, None, None, None, None, None, None, None


class GradChain:
    """The gradient buffer of one dense block's backward: the dx the block's last BN allocated, which every earlier BN of the
    chain then accumulates into in place.  A gradient that is not a prefix view of that very buffer (autograd summed another
    consumer's gradient into a tensor of its own, a caller's grad_output) is never written: that BN allocates afresh."""

    def __init__(self):
        self.buf = None

    def owns(self, g):
        b = self.buf
        return (b is not None and g.data_ptr() == b.data_ptr() and g.stride() == b.stride()
                and g.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and g.shape[3] <= b.shape[3])


class BatchNorm2dNHWC(nn.BatchNorm2d):
    """nn.BatchNorm2d on channels-last fp32 device tensors (kd_bn_nhwc_fwd / kd_bn_nhwc_bwd): batch statistics in train mode,
    running statistics in eval mode, optional fused ReLU (forward(x, relu=True)).  folded() gives the eval-mode
    (scale, shift) a conv epilogue applies instead, cached per version of the parameters and statistics.
    bf16 activations go to kd_bn_nhwc_lp_fwd / _bwd: y and dx are bf16, the parameters, statistics and parameter gradients fp32.
    In either dtype y is allocated by new_padded() and tagged, so a Conv2dNHWC reads its K granule (32 channels in fp32, 64 in bf16)
    in place: the Wide-ResNet's 16-channel stem activation needs no padding copy.  Precomputed statistics
    (forward_with_stats: the DenseNet path) are fp32 only."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._fold = None

    def __deepcopy__(self, memo):
        return _deepcopy_without(self, memo, _fold=None)

    def _check(self, x):
        if not (self.affine and self.track_running_stats) or self.momentum is None:
            raise NotImplementedError("BatchNorm2dNHWC: affine, running statistics, fixed momentum")
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("BatchNorm2dNHWC is fp32 or bf16")

    def folded(self):
        ts = (self.weight, self.bias, self.running_mean, self.running_var)
        key = tuple((t._version, t.data_ptr()) for t in ts) + (self.eps,)
        if self._fold is None or self._fold[0] != key:
            self._fold = (key, ops.bn_fold(self))
        return self._fold[1]

    def _apply_fn(self, x, relu, shortcut, stats=None, chain=None):
        self._check(x)
        if self.training:
            self.num_batches_tracked.add_(1)
        if x.dtype != torch.float32 and stats is not None:
            raise TypeError("BatchNorm2dNHWC: precomputed statistics are fp32 only")
        out = _BatchNormNHWCFn.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.training,
                                     float(self.momentum), float(self.eps), bool(relu), shortcut, stats, chain)
        mark_padded(out[0] if shortcut else out)
        return out

    def forward(self, x, relu=False, stats=None):
        """stats: (mean, invstd, var_unbiased) of x's channels when the caller has them (see forward_with_stats); device only."""
        if _host(x):
            y = super().forward(x)
            return F.relu(y) if relu else y
        return self._apply_fn(x, relu, False, stats if self.training else None)

    def forward_with_shortcut(self, x, relu=False):
        """(forward(x, relu), s) where s is x for an identity shortcut: the gradient reaching s joins dx inside kd_bn_nhwc_bwd
        (its `res` operand).  Not a module call: forward hooks of this BN do not fire."""
        if _host(x):
            return self.forward(x, relu), x
        return self._apply_fn(x, relu, True)

    def forward_with_stats(self, x, stats, relu=False, shortcut=False, chain=None):
        """forward(x, relu) in train mode from batch statistics the caller already has: stats = (mean, invstd, var_unbiased) of
        x's channels (ops.bn_nhwc_stats with this BN's eps) -- one elementwise pass, the running statistics and
        num_batches_tracked updated as forward() does; stats=None (or eval mode) is forward() itself.  shortcut=True returns
        (y, s) as forward_with_shortcut; `chain` (a GradChain) lets a dense block's backward accumulate in one buffer.
        Device tensors only, and not a module call: forward hooks of this BN do not fire."""
        if _host(x):
            raise KdccError("BatchNorm2dNHWC.forward_with_stats takes device tensors")
        return self._apply_fn(x, relu, bool(shortcut), stats if self.training else None, chain)


class _MaxPool3x3s2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xh = _nhwc(x)
        ctx.save_for_backward(xh)
        return ops.maxpool3x3s2(xh)[0].permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        (xh,) = ctx.saved_tensors
        return ops.maxpool3x3s2_bwd(xh, _nhwc(gy)).permute(0, 3, 1, 2)


class MaxPool3x3s2NHWC(nn.MaxPool2d):
    """nn.MaxPool2d(3, 2, 1) on channels-last fp32 device tensors: kd_maxpool3x3s2 / kd_maxpool3x3s2_bwd (C % 8 == 0)."""

    def forward(self, x):
        if _host(x):
            return super().forward(x)
        if (_one(self.kernel_size), _one(self.stride), _one(self.padding), _one(self.dilation)) != (3, 2, 1, 1) or self.ceil_mode \
                or self.return_indices:
            raise NotImplementedError("MaxPool3x3s2NHWC: kernel 3, stride 2, padding 1 only")
        if x.dtype != torch.float32:
            raise TypeError("MaxPool3x3s2NHWC is fp32")
        return _MaxPool3x3s2Fn.apply(x)


class _AvgPool2x2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.size = tuple(x.shape[2:])
        return ops.avgpool2x2(_nhwc(x)).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        return ops.avgpool2x2_bwd(_nhwc(gy), ctx.size).permute(0, 3, 1, 2)


class AvgPool2x2NHWC(nn.AvgPool2d):
    """nn.AvgPool2d(2, 2) on channels-last fp32 device tensors: kd_avgpool2x2_nhwc / kd_avgpool2x2_nhwc_bwd."""

    def forward(self, x):
        if _host(x):
            return super().forward(x)
        if (_one(self.kernel_size), _one(self.stride), _one(self.padding)) != (2, 2, 0) or self.ceil_mode or self.divisor_override:
            raise NotImplementedError("AvgPool2x2NHWC: kernel 2, stride 2, no padding only")
        if x.dtype != torch.float32:
            raise TypeError("AvgPool2x2NHWC is fp32")
        return _AvgPool2x2Fn.apply(x)


# ------------------------------------------------------------------ classifier head of the CIFAR PreResNet (csrc/head_ops.hip)
class _HeadBNReLUPoolFn(torch.autograd.Function):
    """pooled (N,C) = mean over the map of relu(bn(x)): kd_head_bn_relu_pool_fwd reads x once and stores no activation; the
    backward (kd_head_bn_relu_pool_bwd) recomputes the activation's sign from x.  Train mode takes the batch statistics from
    ops.bn_nhwc_stats first; the forward kernel then updates the running statistics as kd_bn_nhwc_apply does."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps):
        xh = _nhwc(x)
        g, b = gamma.contiguous(), beta.contiguous()
        if training:
            mean, invstd, var = ops.bn_nhwc_stats(xh, eps)
            pooled = ops.head_bn_relu_pool_fwd(xh, g, b, mean, invstd, var, running_mean, running_var, momentum)
        else:
            mean, invstd = running_mean, torch.rsqrt(running_var + eps)
            pooled = ops.head_bn_relu_pool_fwd(xh, g, b, mean, invstd)
        ctx.save_for_backward(xh, g, b, mean, invstd)
        ctx.training = training
        return pooled

    @staticmethod
    def backward(ctx, gp):
        xh, g, b, mean, invstd = ctx.saved_tensors
        dx, dg, db = ops.head_bn_relu_pool_bwd(xh, gp.contiguous(), g, b, mean, invstd, ctx.training, need_dx=ctx.needs_input_grad[0])
        return (None if dx is None else dx.permute(0, 3, 1, 2), dg if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None, None, None, None, None, None)


def bn_relu_avgpool(bn, relu, x, kernel_size=8):
    """flatten(AvgPool2d(kernel_size)(relu(bn(x)))) -> (N, C * pooled positions), the tail of the CIFAR PreResNet.  One fused pass
    (_HeadBNReLUPoolFn) when the pool covers the whole map, x is an fp32 device tensor, bn a BatchNorm2dNHWC and neither bn nor relu
    carries a forward hook; otherwise bn(x, relu=True) followed by F.avg_pool2d.  Host tensors (allow_host_tensors) run the modules."""
    if _host(x):
        return F.avg_pool2d(relu(bn(x)), kernel_size).flatten(1)
    if type(bn) is not BatchNorm2dNHWC:     # (a replaced BN: called as a module; the small-shape BatchNorm2d fuses its ReLU)
        return F.avg_pool2d(bn(x, relu=True) if type(bn) is BatchNorm2d else relu(bn(x)), kernel_size).flatten(1)
    if _hooked(bn, relu) or x.dtype != torch.float32 or tuple(x.shape[2:]) != (kernel_size, kernel_size):
        return F.avg_pool2d(bn(x, relu=True).float(), kernel_size).flatten(1)
    bn._check(x)
    if bn.training:
        bn.num_batches_tracked.add_(1)
    return _HeadBNReLUPoolFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, float(bn.momentum), float(bn.eps))


# ------------------------------------------------------------------ BN -> ReLU -> MaxPool2d(2, 2) of the CIFAR VGGs (csrc/pool_ops.hip)
class _BNReLUMaxPoolFn(torch.autograd.Function):
    """(N,C,H//2,W//2) = max over every 2x2 window of relu(bn(x)): kd_bn_relu_maxpool2x2_fwd reads x once and stores the pooled map
    only; the backward (kd_bn_relu_maxpool2x2_bwd) recomputes the windows from x, so nothing but x and the statistics is kept.
    gamma = None: max(relu(x)), the plain VGGs' and the fused eval chain's.  Train mode takes the batch statistics from
    ops.bn_nhwc_stats first; the forward kernel then updates the running statistics as kd_bn_nhwc_apply does.  The pooled map comes
    from new_padded() (the caller tags it)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps):
        xh = _nhwc(x)
        N, H, W, Cc = xh.shape
        out = new_padded((N, H // 2, W // 2, Cc), xh.device)
        if gamma is None:
            g = b = mean = invstd = None
            ops.bn_relu_maxpool2x2_fwd(xh, out=out)
        else:
            g, b = gamma.contiguous(), beta.contiguous()
            if training:
                mean, invstd, var = ops.bn_nhwc_stats(xh, eps)
                ops.bn_relu_maxpool2x2_fwd(xh, g, b, mean, invstd, var, running_mean, running_var, momentum, out=out)
            else:
                mean, invstd = running_mean, torch.rsqrt(running_var + eps)
                ops.bn_relu_maxpool2x2_fwd(xh, g, b, mean, invstd, out=out)
        ctx.save_for_backward(xh, g, b, mean, invstd)
        ctx.training = training
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        xh, g, b, mean, invstd = ctx.saved_tensors
        dx, dg, db = ops.bn_relu_maxpool2x2_bwd(xh, _nhwc(gy), g, b, mean, invstd, ctx.training, need_dx=ctx.needs_input_grad[0] or g is None)
        return (dx.permute(0, 3, 1, 2) if ctx.needs_input_grad[0] else None, dg if ctx.needs_input_grad[1] else None,
                db if ctx.needs_input_grad[2] else None, None, None, None, None, None)


def _plain_maxpool2x2(pool):
    return (type(pool) is nn.MaxPool2d and _one(pool.kernel_size) == 2 and _one(pool.stride) == 2 and _one(pool.padding) == 0
            and _one(pool.dilation) == 1 and not pool.ceil_mode and not pool.return_indices)


# The fused tail with BatchNorm takes maps of at least this many elements.  Below it every version is bound by its launches, not by
# memory, and the fused one has a call more (the batch statistics are a call of their own): at batch 128 it held at vgg16_bn's
# 32x32x64 ... 4x4x512 stages and lost at 2x2x512 (profiles/vgg.md), which therefore takes bn(x, relu=True) + the pool module.
POOL_FUSE_MIN_ELEMENTS = 1 << 20


def call_relu(relu, x):
    """relu(x) as a module call (its hooks fire).  An in-place ReLU may not write into the view an autograd Function of this file
    returned (torch refuses it), so under autograd it gets a copy."""
    if getattr(relu, "inplace", False) and torch.is_grad_enabled() and x.requires_grad:
        x = x.clone()
    return relu(x)


def bn_relu_maxpool(bn, relu, pool, x):
    """pool(relu(bn(x))) for a MaxPool2d(2, 2), the end of every VGG stage; bn = None: pool(relu(x)).  One fused pass
    (_BNReLUMaxPoolFn) when x is an fp32 device tensor, bn a BatchNorm2dNHWC (or None), pool a MaxPool2d(2, 2) without padding,
    dilation, ceil_mode or return_indices, the map holds a window (with a BatchNorm: POOL_FUSE_MIN_ELEMENTS elements), and none of
    the modules carries a forward hook; otherwise the modules are called, bn with its fused ReLU where it has one and relu carries
    no hook.  Host tensors (allow_host_tensors) run the modules."""
    if _host(x):
        return pool(relu(x if bn is None else bn(x)))
    mods = (relu, pool) if bn is None else (bn, relu, pool)
    if (type(bn) in (BatchNorm2dNHWC, type(None)) and type(relu) is nn.ReLU and _plain_maxpool2x2(pool) and not _hooked(*mods)
            and x.dtype == torch.float32 and x.dim() == 4 and x.shape[2] >= 2 and x.shape[3] >= 2
            and (bn is None or x.numel() >= POOL_FUSE_MIN_ELEMENTS)):
        if bn is None:
            return mark_padded(_BNReLUMaxPoolFn.apply(x, None, None, None, None, False, 0.0, 0.0))
        bn._check(x)
        if bn.training:
            bn.num_batches_tracked.add_(1)
        return mark_padded(_BNReLUMaxPoolFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, float(bn.momentum),
                                                  float(bn.eps)))
    if bn is None:
        return pool(call_relu(relu, x))
    if isinstance(bn, (BatchNorm2dNHWC, BatchNorm2d)) and not _hooked(relu):
        return pool(bn(x, relu=True))
    return pool(call_relu(relu, bn(x)))


# ------------------------------------------------------------------ dropout (csrc/dropout.hip; the rule: csrc/dropout_rng.h)
# One process-wide stream (seed, next offset).  A forward draw takes the pair and advances the offset by one; the mask of the call
# is a pure function of the pair and the element's index, so the backward regenerates it from the pair alone.  The seed follows
# torch's: torch.initial_seed() is read at each draw, and when it has changed since the previous draw -- torch.manual_seed(s) before
# a run -- the stream restarts at (s, 0), so seeding torch fixes every mask of the run.  seed_dropout() sets the pair directly and
# holds until torch's seed changes next.  The stream is per process and knows nothing of ranks: ranks seeded alike draw the same
# masks, as torch.nn.functional.dropout does under torch.manual_seed; seed each rank apart (seed + rank) for independent masks.
_U64 = (1 << 64) - 1
_DROPOUT_STREAM = {"seed": None, "offset": 0, "torch_seed": None}


def _dropout_sync():
    s, ts = _DROPOUT_STREAM, torch.initial_seed() & _U64
    if s["torch_seed"] != ts:
        s.update(seed=ts, offset=0, torch_seed=ts)
    return s


def seed_dropout(seed, offset=0):
    """Set the dropout stream: the next draw uses (seed, offset).  Unsigned 64-bit integers."""
    seed, offset = int(seed), int(offset)
    if not (0 <= seed <= _U64 and 0 <= offset <= _U64):
        raise ValueError("seed_dropout: seed and offset are unsigned 64-bit integers")
    _DROPOUT_STREAM.update(seed=seed, offset=offset, torch_seed=torch.initial_seed() & _U64)


def dropout_state():
    """(seed, next offset): the pair the next forward draw will use."""
    s = _dropout_sync()
    return s["seed"], s["offset"]


def _dropout_draw():
    s = _dropout_sync()
    pair = (s["seed"], s["offset"])
    s["offset"] = (s["offset"] + 1) & _U64
    return pair


def _nhwc_view(t):
    """(N,C,H,W)-logical tensor -> (N,H,W,C) pixel-strided view of any alignment; a copy only when t is not channels_last-strided."""
    v = t.permute(0, 2, 3, 1)
    try:
        ops.nhwc_ld(v)
        return v
    except ValueError:
        return _nhwc(t)


class _DropoutFn(torch.autograd.Function):
    """y = dropout(x) with the mask of (seed, offset); the backward is the same pass over gy.  Only (p, seed, offset) is kept."""

    @staticmethod
    def forward(ctx, x, p, seed, offset, out):
        ctx.set_materialize_grads(False)
        ctx.rule = (p, seed, offset)
        xh = _nhwc_view(x)
        y = new_padded(tuple(xh.shape), xh.device, x.dtype) if out is None else out
        return ops.dropout_nhwc(xh, p, seed, offset, out=y).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        if gy is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        return ops.dropout_nhwc(_nhwc_view(gy), *ctx.rule).permute(0, 3, 1, 2), None, None, None, None


def dropout(x, p, training, out=None):
    """F.dropout(x, p, training) for a channels-last fp32 or bf16 device tensor: one kd_dropout_nhwc pass, and the same pass over the
    gradient in the backward -- no mask and no activation is stored.  The identity (no launch, no draw from the stream) when
    `not training` or p == 0.  Each call draws one offset from the dropout stream (seed_dropout / dropout_state).  The result lives
    in a new_padded() buffer and is tagged, so a Conv2dNHWC reads it in place; out, an (N,H,W,C) view of x's dtype (a channel slice
    of a dense block's buffer), receives it instead.  Out of place by default: a producer that saved its output for its backward
    (a BatchNorm with fused ReLU) must not see it change.  Host tensors raise: the rule is device-only."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout: p = {p} is outside [0, 1)")
    if not training or p == 0.0:
        return x
    if _host(x):
        raise NotImplementedError("nn_hip.dropout: the dropout rule runs on the device only")
    seed, offset = _dropout_draw()
    y = _DropoutFn.apply(x, p, seed, offset, out)
    return mark_padded(y) if out is None else y
