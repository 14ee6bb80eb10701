"""HRNetV2 + OCR (Sun et al.; Yuan et al.; HRNetV2-W48 + OCR is the teacher of cfg/cityscapes/10M_hrnet_all.json) with the
reference's module tree and state-dict keys (models/hrnet_ocr/seg_hrnet_ocr.py): conv1 / bn1 / conv2 / bn2, layer1,
transition1..3, stage2..4 of HighResolutionModule {branches, fuse_layers}, conv3x3_ocr, ocr_gather_head,
ocr_distri_head.{object_context_block.{f_pixel, f_object, f_down, f_up}, conv_bn_dropout}, cls_head, aux_head -- so a checkpoint
loads through forgiving_state_restore and the plan names of the shipped config (stage4.0.branches.3.N.conv1 / conv2) resolve.
Same constructor: HighResolutionNet(config=DEFAULT_CONFIG, **kwargs), extra kwargs (num_classes=19) accepted and ignored.

Channels-last fp32 throughout, as in cifar_models/wrn.py and densenet.py: convolutions are nn_hip.Conv2dNHWCBias (Conv2dNHWC
with pad_channels on: any output channel count, outputs in granule-padded buffers), BatchNorm nn_hip.BatchNorm2dNHWC following
the module's training flag.  What is specific to this network:

  * the exchange unit of a HighResolutionModule -- upsample every coarser branch, add, ReLU -- is one kd_hr_fuse_fwd pass per
    output branch (backward kd_hr_fuse_bwd); the 1x1 conv + BN of a coarser branch and the strided 3x3 chains of a finer one stay
    convolutions.  The residual add + ReLU that closes a BasicBlock / Bottleneck is the same kernel with two sources;
  * the 720-channel concatenation of the four branches is written slice by slice (kd_upsample_bilinear_ac with ldy) into ONE
    buffer whose pixel stride is padded to the conv granule (736) with a zero tail, which aux_head.0 and conv3x3_ocr.0 read in
    place; there is no torch.cat anywhere;
  * SpatialGather_Module is kd_ocr_gather_fwd / _bwd, the contraction core of the object attention block kd_ocr_attend_fwd / _bwd;
  * a tensor whose channel count is no multiple of the conv granule (the 48-channel branch) is produced by the convolutions and
    by the fuse sum in a buffer whose pixel stride is padded to the granule (64) with a zero tail, and the next conv reads it in
    place.  What still takes Conv2dNHWC's padded copy: the output of a BatchNorm that runs as a module (train mode, or behind a
    trainable layer) and, in the backward, the 48-channel output gradient;
  * a frozen conv + eval-mode BN (+ ReLU) whose output nobody hooks and that needs no gradient runs as one conv launch with the
    BN folded into the epilogue (the whole teacher; the student's frozen layers in front of the first trainable one);
  * Dropout2d(0.05) stays torch's op.

Host tensors (nn_hip.allow_host_tensors) run the torch base classes, like the reference.  The compute dtype is fp32 only.
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import nn_hip, ops
from ..nn_hip import BatchNorm2dNHWC, Conv2dNHWCBias, _hooked

__all__ = ["HighResolutionNet", "DEFAULT_CONFIG"]

# the W48 layout, in the schema of the reference's models/hrnet_ocr/config_hrnet_ocr.json (never read from a file at import time)
DEFAULT_CONFIG = {
    "extra": {
        "FINAL_CONV_KERNEL": 1,
        "STAGE1": {"NUM_MODULES": 1, "NUM_RANCHES": 1, "BLOCK": "BOTTLENECK", "NUM_BLOCKS": [4], "NUM_CHANNELS": [64],
                   "FUSE_METHOD": "SUM"},
        "STAGE2": {"NUM_MODULES": 1, "NUM_BRANCHES": 2, "BLOCK": "BASIC", "NUM_BLOCKS": [4, 4], "NUM_CHANNELS": [48, 96],
                   "FUSE_METHOD": "SUM"},
        "STAGE3": {"NUM_MODULES": 4, "NUM_BRANCHES": 3, "BLOCK": "BASIC", "NUM_BLOCKS": [4, 4, 4], "NUM_CHANNELS": [48, 96, 192],
                   "FUSE_METHOD": "SUM"},
        "STAGE4": {"NUM_MODULES": 3, "NUM_BRANCHES": 4, "BLOCK": "BASIC", "NUM_BLOCKS": [4, 4, 4, 4],
                   "NUM_CHANNELS": [48, 96, 192, 384], "FUSE_METHOD": "SUM"},
    },
    "align_corners": True,
    "ocr.mid_channels": 512,
    "ocr.key_channels": 256,
    "num_classes": 19,
}


# ------------------------------------------------------------------------------------------------ autograd wrappers
class _FuseFn(torch.autograd.Function):
    """relu(sum_s sample(src_s)) over NCHW-logical channels-last tensors, added in order; the output has the size of srcs[at]."""

    @staticmethod
    def forward(ctx, at, *srcs):
        hs = [nn_hip._nhwc(s) for s in srcs]
        N, Ho, Wo, Cc = hs[at].shape
        y = ops.hr_fuse(hs, out=nn_hip.new_padded((N, Ho, Wo, Cc), hs[at].device))
        ctx.sizes = [tuple(h.shape[1:3]) for h in hs]
        ctx.save_for_backward(y)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gs = ops.hr_fuse_bwd(nn_hip._nhwc(gy), y, ctx.sizes, ctx.needs_input_grad[1:])
        return (None,) + tuple(None if g is None else g.permute(0, 3, 1, 2) for g in gs)


def fuse_sum(srcs, at=0):
    if nn_hip._host(srcs[0]):
        size = srcs[at].shape[-2:]
        y = None
        for s in srcs:
            s = s if s.shape[-2:] == size else F.interpolate(s, size=size, mode="bilinear", align_corners=True)
            y = s if y is None else y + s
        return F.relu(y)
    return nn_hip.mark_padded(_FuseFn.apply(at, *srcs))


class _GatherFn(torch.autograd.Function):
    """SpatialGather_Module: feats (N,C,H,W), logits (N,K,H,W) -> context (N,C,K,1)."""

    @staticmethod
    def forward(ctx, feats, logits):
        fh, lh = nn_hip._nhwc(feats), nn_hip._nhwc(logits)
        N, H, W, Cc = fh.shape
        f3, l3 = fh.as_strided((N, H * W, Cc), (fh.stride(0), fh.stride(2), 1)), lh.as_strided((N, H * W, lh.shape[3]), (lh.stride(0), lh.stride(2), 1))
        c, _, lse = ops.ocr_gather(l3, f3)
        ctx.save_for_backward(f3, l3, c, lse)
        ctx.hw = (H, W)
        K = c.shape[1]
        return c.as_strided((N, Cc, K, 1), (K * Cc, 1, Cc, Cc))        # (N,K,C) storage seen as a K x 1 channels-last map

    @staticmethod
    def backward(ctx, gc):
        f3, l3, c, lse = ctx.saved_tensors
        H, W = ctx.hw
        g = gc.squeeze(3).permute(0, 2, 1).contiguous()
        df, dl = ops.ocr_gather_bwd(g, c, l3, f3, lse)
        N = df.shape[0]
        return df.view(N, H, W, -1).permute(0, 3, 1, 2), dl.view(N, H, W, -1).permute(0, 3, 1, 2)


class _AttendFn(torch.autograd.Function):
    """query (N,Ck,H,W), key / value (N,Ck,K,1) -> (N,Ck,H,W): softmax_K(Ck^-0.5 query . key^T) . value."""

    @staticmethod
    def forward(ctx, query, key, value):
        qh = nn_hip._nhwc(query)
        N, H, W, Ck = qh.shape
        q3 = qh.as_strided((N, H * W, Ck), (qh.stride(0), qh.stride(2), 1))
        k3, v3 = (nn_hip._nhwc(t).reshape(N, -1, Ck) for t in (key, value))
        ctx.save_for_backward(q3, k3, v3)
        ctx.hw = (H, W)
        return ops.ocr_attend(q3, k3, v3).view(N, H, W, Ck).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        q3, k3, v3 = ctx.saved_tensors
        H, W = ctx.hw
        gh = nn_hip._nhwc(gy)
        N, _, _, Ck = gh.shape
        dq, dk, dv = ops.ocr_attend_bwd(gh.as_strided((N, H * W, Ck), (gh.stride(0), gh.stride(2), 1)), q3, k3, v3)
        back = lambda t: t.permute(0, 2, 1).unsqueeze(3)            # (N,K,Ck) -> (N,Ck,K,1)
        return dq.view(N, H, W, Ck).permute(0, 3, 1, 2), back(dk), back(dv)


class _UpsampleFn(torch.autograd.Function):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) on kd_upsample_bilinear_ac / _bwd."""

    @staticmethod
    def forward(ctx, x, size):
        xh = nn_hip._nhwc(x)
        ctx.in_size = tuple(xh.shape[1:3])
        return ops.upsample_bilinear_ac(xh, size).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        return ops.upsample_bilinear_ac_bwd(nn_hip._nhwc(gy).contiguous(), ctx.in_size).permute(0, 3, 1, 2), None


def upsample(x, size):
    if nn_hip._host(x):
        return F.interpolate(x, size=size, mode="bilinear", align_corners=True)
    return _UpsampleFn.apply(x, tuple(size))


class _ConcatUpFn(torch.autograd.Function):
    """Branch outputs -> their concatenation at the first one's size, each written into its channel slice of one buffer whose
    pixel stride is the conv granule above the channel total (zero tail): the consumers read it without a padded copy."""

    @staticmethod
    def forward(ctx, *xs):
        hs = [nn_hip._nhwc(x) for x in xs]
        N, H, W, _ = hs[0].shape
        buf = nn_hip.new_padded((N, H, W, sum(h.shape[3] for h in hs)), hs[0].device)
        c0 = 0
        for h in hs:
            c1 = c0 + h.shape[3]
            if tuple(h.shape[1:3]) == (H, W):
                nn_hip._copy_into(h, buf[..., c0:c1])
            else:
                ops.upsample_bilinear_ac(h, (H, W), out=buf[..., c0:c1])
            c0 = c1
        ctx.sizes = [tuple(h.shape[1:]) for h in hs]
        return buf.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        g = nn_hip._nhwc(gy)
        outs, c0 = [], 0
        for i, (h, w, c) in enumerate(ctx.sizes):
            gs = g[..., c0:c0 + c]
            c0 += c
            if not ctx.needs_input_grad[i]:
                outs.append(None)
            elif (h, w) == tuple(g.shape[1:3]):
                outs.append(gs.permute(0, 3, 1, 2))
            else:
                outs.append(ops.upsample_bilinear_ac_bwd(gs.contiguous(), (h, w)).permute(0, 3, 1, 2))
        return tuple(outs)


def concat_upsampled(xs):
    if nn_hip._host(xs[0]):
        size = xs[0].shape[-2:]
        return torch.cat([xs[0]] + [F.interpolate(x, size=size, mode="bilinear", align_corners=True) for x in xs[1:]], 1)
    return nn_hip.mark_padded(_ConcatUpFn.apply(*xs))


class _Concat2Fn(torch.autograd.Function):
    """torch.cat([a, b], 1) as two slice copies into one NHWC buffer."""

    @staticmethod
    def forward(ctx, a, b):
        ah, bh = nn_hip._nhwc(a), nn_hip._nhwc(b)
        N, H, W, ca = ah.shape
        buf = torch.empty((N, H, W, ca + bh.shape[3]), dtype=torch.float32, device=ah.device)
        nn_hip._copy_into(ah, buf[..., :ca])
        nn_hip._copy_into(bh, buf[..., ca:])
        ctx.ca = ca
        return buf.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        return gy[:, :ctx.ca], gy[:, ctx.ca:]


def concat2(a, b):
    if nn_hip._host(a):
        return torch.cat([a, b], 1)
    return _Concat2Fn.apply(a, b)


# ------------------------------------------------------------------------------------------------ conv + BN (+ ReLU)
def _needs_graph(x, *mods):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for m in mods for p in m.parameters()))


def conv_bn(conv, bn, x, relu):
    """relu?(bn(conv(x))).  Frozen, eval-mode, un-hooked and outside any autograd graph: one conv launch with the BN folded into
    the epilogue.  Otherwise the two modules are called as modules (hooks fire, a replaced conv runs its own forward)."""
    if (x.is_cuda and type(conv) is Conv2dNHWCBias and type(bn) is BatchNorm2dNHWC and not bn.training
            and not _hooked(conv, bn) and not _needs_graph(x, conv, bn)):
        return conv.run_folded(x, bn, relu)
    y = conv(x)
    if isinstance(bn, BatchNorm2dNHWC):
        return bn(y, relu=relu)
    y = bn(y)
    return F.relu(y) if relu else y


class _ConvBN(nn.Sequential):
    """Sequential(conv, bn[, relu]) with the reference's child indices, run through conv_bn()."""

    def __init__(self, conv, bn, relu):
        super().__init__(conv, bn, *([nn.ReLU(inplace=True)] if relu else []))

    def forward(self, x):
        return conv_bn(self[0], self[1], x, len(self) > 2)


class _BNReLU(nn.Sequential):
    """The reference's ModuleHelper.BNReLU: Sequential(BatchNorm2d, ReLU) -- the BN is child 0."""

    def __init__(self, num_features):
        super().__init__(BatchNorm2dNHWC(num_features), nn.ReLU())


class _ConvBNReLUChain(nn.Sequential):
    """Sequential(conv, BNReLU, [conv, BNReLU, ...][, Dropout2d]): the OCR block's transforms, each pair one conv_bn()."""

    def forward(self, x):
        mods = list(self.children())
        i = 0
        while i < len(mods):
            if isinstance(mods[i], nn.Conv2d) and i + 1 < len(mods) and isinstance(mods[i + 1], _BNReLU):
                x = conv_bn(mods[i], mods[i + 1][0], x, True)
                i += 2
            else:
                x = mods[i](x)
                i += 1
        return x


# (the pad_channels flavour for every layer: its backward takes output channel counts that are no multiple of 32 -- 48, and
# the narrow test configs' 16 -- which the dense flavour's input gradient does not)
def _conv3x3(cin, cout, stride=1):
    return Conv2dNHWCBias(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False)


def _conv1x1(cin, cout):
    return Conv2dNHWCBias(cin, cout, kernel_size=1, stride=1, padding=0, bias=False)


# ------------------------------------------------------------------------------------------------ residual blocks
class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv3x3(inplanes, planes, stride)
        self.bn1 = BatchNorm2dNHWC(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _conv3x3(planes, planes)
        self.bn2 = BatchNorm2dNHWC(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = conv_bn(self.conv1, self.bn1, x, True)
        out = conv_bn(self.conv2, self.bn2, out, False)
        residual = x if self.downsample is None else self.downsample(x)
        return fuse_sum([out, residual])


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv1x1(inplanes, planes)
        self.bn1 = BatchNorm2dNHWC(planes)
        self.conv2 = _conv3x3(planes, planes, stride)
        self.bn2 = BatchNorm2dNHWC(planes)
        self.conv3 = _conv1x1(planes, planes * self.expansion)
        self.bn3 = BatchNorm2dNHWC(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = conv_bn(self.conv1, self.bn1, x, True)
        out = conv_bn(self.conv2, self.bn2, out, True)
        out = conv_bn(self.conv3, self.bn3, out, False)
        residual = x if self.downsample is None else self.downsample(x)
        return fuse_sum([out, residual])


blocks_dict = {"BASIC": BasicBlock, "BOTTLENECK": Bottleneck}


def _make_blocks(block, inplanes, planes, count, stride=1):
    downsample = None
    if stride != 1 or inplanes != planes * block.expansion:
        downsample = _ConvBN(Conv2dNHWCBias(inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                             BatchNorm2dNHWC(planes * block.expansion), relu=False)
    layers = [block(inplanes, planes, stride, downsample)]
    layers += [block(planes * block.expansion, planes) for _ in range(1, count)]
    return nn.Sequential(*layers)


# ------------------------------------------------------------------------------------------------ the exchange module
class HighResolutionModule(nn.Module):
    def __init__(self, num_branches, blocks, num_blocks, num_inchannels, num_channels, fuse_method, multi_scale_output=True):
        super().__init__()
        for what, lst in (("NUM_BLOCKS", num_blocks), ("NUM_CHANNELS", num_channels), ("NUM_INCHANNELS", num_inchannels)):
            if num_branches != len(lst):
                raise ValueError("NUM_BRANCHES({}) <> {}({})".format(num_branches, what, len(lst)))
        self.num_branches = num_branches
        self.fuse_method = fuse_method
        self.multi_scale_output = multi_scale_output
        self.branches = nn.ModuleList(_make_blocks(blocks, num_inchannels[i], num_channels[i], num_blocks[i]) for i in range(num_branches))
        self.num_inchannels = [num_channels[i] * blocks.expansion for i in range(num_branches)]
        self.fuse_layers = self._make_fuse_layers()
        self.relu = nn.ReLU(inplace=True)

    def _make_fuse_layers(self):
        if self.num_branches == 1:
            return None
        ch = self.num_inchannels
        rows = []
        for i in range(self.num_branches if self.multi_scale_output else 1):
            row = []
            for j in range(self.num_branches):
                if j > i:          # coarser branch: 1x1 conv + BN here, the upsample belongs to the fuse kernel
                    row.append(_ConvBN(_conv1x1(ch[j], ch[i]), BatchNorm2dNHWC(ch[i]), relu=False))
                elif j == i:
                    row.append(None)
                else:              # finer branch: i - j strided 3x3 convs, the last one onto this branch's channels, without ReLU
                    steps = i - j
                    row.append(nn.Sequential(*[
                        _ConvBN(_conv3x3(ch[j], ch[i] if k == steps - 1 else ch[j], 2),
                                BatchNorm2dNHWC(ch[i] if k == steps - 1 else ch[j]), relu=k != steps - 1)
                        for k in range(steps)]))
            rows.append(nn.ModuleList(row))
        return nn.ModuleList(rows)

    def get_num_inchannels(self):
        return self.num_inchannels

    def forward(self, x):
        if self.num_branches == 1:
            return [self.branches[0](x[0])]
        x = [self.branches[i](x[i]) for i in range(self.num_branches)]
        fused = []
        for i, row in enumerate(self.fuse_layers):
            srcs = [x[j] if j == i else row[j](x[j]) for j in range(self.num_branches)]
            fused.append(fuse_sum(srcs, at=i))
        return fused


# ------------------------------------------------------------------------------------------------ OCR head
class SpatialGather_Module(nn.Module):
    """Soft class regions: context[n, :, k] = sum_hw softmax_hw(scale * probs[n, k]) * feats[n, :, hw]."""

    def __init__(self, cls_num=0, scale=1):
        super().__init__()
        self.cls_num = cls_num
        self.scale = scale

    def forward(self, feats, probs):
        if nn_hip._host(feats):
            n, k = probs.shape[:2]
            p = F.softmax(self.scale * probs.reshape(n, k, -1), dim=2)
            return torch.matmul(p, feats.reshape(n, feats.shape[1], -1).permute(0, 2, 1)).permute(0, 2, 1).unsqueeze(3)
        if self.scale != 1:
            probs = probs * self.scale
        return _GatherFn.apply(feats, probs)


class _ObjectAttentionBlock(nn.Module):
    def __init__(self, in_channels, key_channels, scale=1, bn_type=None):
        super().__init__()
        if scale != 1:
            raise NotImplementedError("object attention: scale > 1 (pooled queries) is not used by any shipped config")
        self.scale = scale
        self.in_channels = in_channels
        self.key_channels = key_channels
        self.pool = nn.MaxPool2d(kernel_size=(scale, scale))
        two = lambda: _ConvBNReLUChain(_conv1x1(in_channels, key_channels), _BNReLU(key_channels),
                                       _conv1x1(key_channels, key_channels), _BNReLU(key_channels))
        self.f_pixel = two()
        self.f_object = two()
        self.f_down = _ConvBNReLUChain(_conv1x1(in_channels, key_channels), _BNReLU(key_channels))
        self.f_up = _ConvBNReLUChain(_conv1x1(key_channels, in_channels), _BNReLU(in_channels))

    def forward(self, x, proxy):
        query, key, value = self.f_pixel(x), self.f_object(proxy), self.f_down(proxy)
        if nn_hip._host(x):
            n, ck = query.shape[:2]
            sim = torch.matmul(query.reshape(n, ck, -1).permute(0, 2, 1), key.reshape(n, ck, -1)) * self.key_channels ** -.5
            ctx = torch.matmul(F.softmax(sim, dim=-1), value.reshape(n, ck, -1).permute(0, 2, 1))
            context = ctx.permute(0, 2, 1).reshape(n, ck, *x.shape[2:])
        else:
            context = _AttendFn.apply(query, key, value)
        return self.f_up(context)


class ObjectAttentionBlock2D(_ObjectAttentionBlock):
    pass


class SpatialOCR_Module(nn.Module):
    def __init__(self, in_channels, key_channels, out_channels, scale=1, dropout=0.1, bn_type=None):
        super().__init__()
        self.object_context_block = ObjectAttentionBlock2D(in_channels, key_channels, scale, bn_type)
        self.conv_bn_dropout = _ConvBNReLUChain(_conv1x1(2 * in_channels, out_channels), _BNReLU(out_channels), nn.Dropout2d(dropout))

    def forward(self, feats, proxy_feats):
        context = self.object_context_block(feats, proxy_feats)
        return self.conv_bn_dropout(concat2(context, feats))


class _AuxHead(nn.Sequential):
    """Sequential(conv 1x1 + bias, BN, ReLU, conv 1x1 + bias onto the classes)."""

    def forward(self, x):
        return self[3](conv_bn(self[0], self[1], x, True))


# ------------------------------------------------------------------------------------------------ the network
class HighResolutionNet(nn.Module):
    def __init__(self, config=DEFAULT_CONFIG, **kwargs):
        super().__init__()
        config = copy.deepcopy(config)
        extra = config["extra"]
        if not config.get("align_corners", True):
            raise NotImplementedError("HighResolutionNet: align_corners = false is not used by any shipped config")
        self.conv1 = _conv3x3(3, 64, 2)
        self.bn1 = BatchNorm2dNHWC(64)
        self.conv2 = _conv3x3(64, 64, 2)
        self.bn2 = BatchNorm2dNHWC(64)
        self.relu = nn.ReLU(inplace=True)

        self.stage1_cfg = extra["STAGE1"]
        block = blocks_dict[self.stage1_cfg["BLOCK"]]
        planes = self.stage1_cfg["NUM_CHANNELS"][0]
        self.layer1 = _make_blocks(block, 64, planes, self.stage1_cfg["NUM_BLOCKS"][0])
        pre = [block.expansion * planes]

        for idx in (2, 3, 4):
            cfg = extra["STAGE%d" % idx]
            setattr(self, "stage%d_cfg" % idx, cfg)
            block = blocks_dict[cfg["BLOCK"]]
            channels = [c * block.expansion for c in cfg["NUM_CHANNELS"]]
            setattr(self, "transition%d" % (idx - 1), self._make_transition_layer(pre, channels))
            stage, pre = self._make_stage(cfg, channels)
            setattr(self, "stage%d" % idx, stage)

        last = int(sum(pre))
        mid, key, ncls = config["ocr.mid_channels"], config["ocr.key_channels"], config["num_classes"]
        self.conv3x3_ocr = _ConvBN(Conv2dNHWCBias(last, mid, kernel_size=3, stride=1, padding=1), BatchNorm2dNHWC(mid), relu=True)
        self.ocr_gather_head = SpatialGather_Module(ncls)
        self.ocr_distri_head = SpatialOCR_Module(in_channels=mid, key_channels=key, out_channels=mid, scale=1, dropout=0.05)
        self.cls_head = Conv2dNHWCBias(mid, ncls, kernel_size=1, stride=1, padding=0, bias=True)
        self.aux_head = _AuxHead(Conv2dNHWCBias(last, last, kernel_size=1, stride=1, padding=0), BatchNorm2dNHWC(last),
                                 nn.ReLU(inplace=True), Conv2dNHWCBias(last, ncls, kernel_size=1, stride=1, padding=0, bias=True))

    @staticmethod
    def _make_transition_layer(pre, cur):
        layers = []
        for i, c in enumerate(cur):
            if i < len(pre):
                layers.append(_ConvBN(_conv3x3(pre[i], c), BatchNorm2dNHWC(c), relu=True) if c != pre[i] else None)
            else:                  # a new, coarser branch: strided 3x3 convs from the coarsest existing one
                steps = i + 1 - len(pre)
                layers.append(nn.Sequential(*[
                    _ConvBN(_conv3x3(pre[-1], c if j == steps - 1 else pre[-1], 2), BatchNorm2dNHWC(c if j == steps - 1 else pre[-1]), relu=True)
                    for j in range(steps)]))
        return nn.ModuleList(layers)

    @staticmethod
    def _make_stage(cfg, num_inchannels, multi_scale_output=True):
        block = blocks_dict[cfg["BLOCK"]]
        modules = []
        for i in range(cfg["NUM_MODULES"]):
            multi = multi_scale_output or i != cfg["NUM_MODULES"] - 1
            modules.append(HighResolutionModule(cfg["NUM_BRANCHES"], block, cfg["NUM_BLOCKS"], num_inchannels, cfg["NUM_CHANNELS"],
                                                cfg["FUSE_METHOD"], multi))
            num_inchannels = modules[-1].get_num_inchannels()
        return nn.Sequential(*modules), num_inchannels

    @staticmethod
    def _transition(layers, ys, prev_branches):
        return [ys[i] if t is None else t(ys[i] if i < prev_branches else ys[-1]) for i, t in enumerate(layers)]

    def forward(self, x):
        if not nn_hip._host(x) and x.dtype != torch.float32:
            raise TypeError("HighResolutionNet is fp32 (bf16 is not implemented for this network)")
        size = tuple(x.shape[-2:])
        x = conv_bn(self.conv1, self.bn1, x, True)
        x = conv_bn(self.conv2, self.bn2, x, True)
        x = self.layer1(x)
        ys = self.stage2(self._transition(self.transition1, [x], 1))
        ys = self.stage3(self._transition(self.transition2, ys, self.stage2_cfg["NUM_BRANCHES"]))
        ys = self.stage4(self._transition(self.transition3, ys, self.stage3_cfg["NUM_BRANCHES"]))

        feats = concat_upsampled(ys)
        out_aux = self.aux_head(feats)
        feats = self.conv3x3_ocr(feats)
        context = self.ocr_gather_head(feats, out_aux)
        feats = self.ocr_distri_head(feats, context)
        return upsample(self.cls_head(feats), size)

    def init_weights(self, pretrained=""):
        """Normal(0, 0.001) convs and unit BatchNorm outside the OCR / class heads, then the checkpoint named by the config."""
        import os
        for name, m in self.named_modules():
            if any(part in name for part in ("cls", "aux", "ocr")):
                continue
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.001)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if os.path.isfile(pretrained):
            loaded = torch.load(pretrained, map_location="cpu")
            loaded = {k.replace("last_layer", "aux_head").replace("model.", ""): v for k, v in loaded.items()}
            own = self.state_dict()
            own.update({k: v for k, v in loaded.items() if k in own})
            self.load_state_dict(own)
        elif pretrained:
            raise RuntimeError("No such file {}".format(pretrained))
