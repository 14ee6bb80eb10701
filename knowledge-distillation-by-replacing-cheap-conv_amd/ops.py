"""Tensor-level wrappers over the C-ABI (include/kdcc.h).

Activations are torch tensors of logical shape (N, H, W, C) whose last
dimension is dense and whose pixel stride `ld` may exceed C (a channel slice of
a wider NHWC buffer).  Every function validates shapes on the host before a
kernel is launched and enqueues on torch's current HIP stream.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import (KD_BF16, KD_F32, KD_PACK_DGRAD, KD_PACK_FWD, ConvDesc, ConvEpilogue, DConvDesc, DwDesc, DwEpilogue, MultiTargets, View3,
                   check)


# Optional live profiler (bench.py): a list that receives (family, algorithmic work, start event, end event, label, device
# kernel the dispatcher picked) for every launch of the conv / depthwise / weight-gradient / loss entry points, the events
# recorded on the stream the kernel is launched on.  Work is algorithmic FLOPs for the MFMA-bound families ("conv_igemm",
# "conv_wgrad", "pw_wgrad") and algorithmic HBM bytes -- every operand read once, every result written once -- for the
# HBM-bound ones ("depthwise", "loss").
PROFILER = None


def _prof_start():
    if PROFILER is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _prof_stop(e0, family, work, label, kernel=None):
    if e0 is None or PROFILER is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    PROFILER.append((family, float(work), e0, e1, label, kernel if kernel is not None else _lib.last_kernel()))


def _nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


# Every buffer that is handed to the library and is not a result comes from _ws (bytes) or _scratch (typed): the one seam the
# tests replace to hand the kernels poisoned, guarded memory (tests/_scratch.py).  Nothing is cleared here: no kernel may
# depend on what its scratch held before the call.  (Results a wrapper returns are plain torch.empty.)
def _ws(nbytes, device, floor=16):
    return torch.empty(max(int(nbytes), floor), dtype=torch.uint8, device=device)


def _scratch(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def dt_of(t):
    if t.dtype == torch.bfloat16:
        return KD_BF16
    if t.dtype == torch.float32:
        return KD_F32
    raise TypeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    if type(t) is not torch.Tensor and hasattr(t, "materialize"):   # lazy.LazyLogits has no storage of its own
        t = t.materialize()
    return C.c_void_p(t.data_ptr())


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.KdccError("kdcc kernels need device tensors (there is no CPU fallback)")


def nhwc_ld(t):
    """Pixel stride of an (N,H,W,C) activation view; validates the layout."""
    if t.dim() != 4 or t.stride(3) != 1:
        raise ValueError(f"expected an (N,H,W,C) tensor with dense channels, got shape {tuple(t.shape)} stride {t.stride()}")
    N, H, W, _ = t.shape
    ld = t.stride(2)
    if (W > 1 and ld < t.shape[3]) or (H > 1 and t.stride(1) != W * ld) or (N > 1 and t.stride(0) != H * W * ld):
        raise ValueError(f"not a pixel-strided NHWC view: shape {tuple(t.shape)} stride {t.stride()}")
    return ld


def new_nhwc(N, H, W, Cc, dtype, device, zero=False):
    f = torch.zeros if zero else torch.empty
    return f((N, H, W, Cc), dtype=dtype, device=device)


def as_nchw(t):
    """(N,H,W,C) activation -> logical NCHW view (channels_last memory), no copy."""
    return t.permute(0, 3, 1, 2)


def conv_out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


# ------------------------------------------------------------------------------ dense conv
def pack_conv_weight(w, dtype, mode=KD_PACK_FWD, cin_pad=None):
    """nn.Conv2d.weight (Cout,Cin,kh,kw) fp32 -> packed operand for conv2d()."""
    _need_cuda(w)
    w = w.detach().contiguous().float()
    Cout, Cin, kh, kw = w.shape
    cin_pad = Cin if cin_pad is None else cin_pad
    if mode == KD_PACK_FWD:
        out = torch.empty((Cout, kh, kw, cin_pad), dtype=dtype, device=w.device)
    else:
        out = torch.empty((Cin, kh, kw, Cout), dtype=dtype, device=w.device)
    check(_lib.lib().kd_pack_conv_weight(_ptr(w), _ptr(out), dt_of(out), mode, Cout, Cin, kh, kw, cin_pad, stream_ptr()),
          "kd_pack_conv_weight")
    return out


class DualUnsupported(_lib.KdccError):
    """conv2d(..., x2=...) on a shape the K-concatenated 1x1 kernel does not take: run the two convs instead."""


class ClsUnsupported(_lib.KdccError):
    """conv2d(..., cls_w=, cls_out=) on a problem whose kernel does not carry the classifier epilogue: store the activation and run the 1x1."""


def conv2d(x, w_packed, stride=1, pad=0, dil=1, *, res_pre=None, mask=None, mask_scale=None, res_post=None,
           out_raw=None, out_act=None, act_scale=None, act_shift=None, act_relu=False, algo_cin=None, algo_cout=None, bn_sums=None,
           x2=None, out_sums=None, cls_w=None, cls_out=None):
    """Implicit-GEMM conv; w_packed is (Cout,kh,kw,Cin). Outputs are caller-provided NHWC views.
    cls_w / cls_out: a (32,1,1,Cout) packed 1x1 classifier (rows >= ncls zero: pack_conv_weight of the weight padded to 32 outputs) and a
    (N,Ho,Wo,ncls) fp32 tensor: the classifier is applied to the activation act(scale * v + shift) in the conv's epilogue INSTEAD of storing
    it (no out_raw / out_act); raises ClsUnsupported where conv_cls_ok() is false.
    x2: a second (N,H,W,Cin2) source of a K-concatenated 1x1 conv -- w_packed is then (Cout,1,1,Cin + Cin2), the result
    [x | x2] . w^T in one accumulator chain (kd_conv1x1_dual_fwd); raises DualUnsupported where the kernel does not apply.
    bn_sums: an empty list (backward, with `mask`): when the kernel this problem selects can take the eval-BN parameter sums in
    its epilogue, (s1, s2) = per-channel sums of the masked gradient and of it times `mask` are appended -- what
    channel_sums(out_raw, sub=res_post, a=mask) would return from another pass over the tensors; otherwise it stays empty.
    out_sums: an empty list (forward, no epilogue operand, out_raw alone): when the selected kernel can sum its output per channel
    over blocks of 128 pixels in its epilogue, the [M/128][2][Cout] partial rows are appended (aspp_image_pool(..., sums=) takes
    them: the global average pool of the tensor without another pass over it); otherwise, and when the call raises, it stays empty."""
    _need_cuda(x, w_packed)
    N, H, W, Cin = x.shape
    Cout, kh, kw, Cin_w = w_packed.shape
    Cin2 = 0
    if x2 is not None:
        _need_cuda(x2)
        if tuple(x2.shape[:3]) != (N, H, W) or x2.dtype != x.dtype or (kh, kw, stride, pad) != (1, 1, 1, 0):
            raise ValueError("conv2d: x2 needs a 1x1 / stride-1 conv and a source of the same pixels and dtype")
        Cin2 = x2.shape[3]
    if Cin_w != Cin + Cin2:
        raise ValueError(f"conv2d: input has {Cin + Cin2} channels, packed weight expects {Cin_w}")
    if w_packed.dtype != x.dtype or not w_packed.is_contiguous():
        raise ValueError("conv2d: packed weight must be contiguous and of the activation dtype")
    Ho, Wo = conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil)
    d = ConvDesc(dt_of(x), N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil, nhwc_ld(x))
    ep = ConvEpilogue()

    def chk(t, name, f32_ok=False):
        if t is None:
            return 0
        if tuple(t.shape) != (N, Ho, Wo, Cout):
            raise ValueError(f"conv2d: {name} has shape {tuple(t.shape)}, expected {(N, Ho, Wo, Cout)}")
        if t.dtype != x.dtype and not (f32_ok and t.dtype == torch.float32):
            raise ValueError(f"conv2d: {name} dtype {t.dtype} != {x.dtype}")
        _need_cuda(t)
        return nhwc_ld(t)

    def chk_vec(v, name):
        if v is not None and (v.dtype != torch.float32 or v.numel() != Cout or not v.is_contiguous()):
            raise ValueError(f"conv2d: {name} must be a contiguous fp32 vector of {Cout}")
        _need_cuda(v)

    ep.res_pre, ep.ld_res_pre = _ptr(res_pre), chk(res_pre, "res_pre")
    ep.mask, ep.ld_mask = _ptr(mask), chk(mask, "mask")
    chk_vec(mask_scale, "mask_scale"); ep.mask_scale = _ptr(mask_scale)
    ep.res_post, ep.ld_res_post = _ptr(res_post), chk(res_post, "res_post")
    ep.out_raw, ep.ld_raw = _ptr(out_raw), chk(out_raw, "out_raw", f32_ok=True)
    ep.raw_f32 = int(out_raw is not None and out_raw.dtype == torch.float32 and x.dtype != torch.float32)
    ep.out_act, ep.ld_act = _ptr(out_act), chk(out_act, "out_act")
    chk_vec(act_scale, "act_scale"); chk_vec(act_shift, "act_shift")
    ep.act_scale, ep.act_shift, ep.act_relu = _ptr(act_scale), _ptr(act_shift), int(act_relu)
    ep.bn_sums = None
    if (cls_w is None) != (cls_out is None):
        raise ValueError("conv2d: cls_w and cls_out come together")
    if cls_w is not None:
        _need_cuda(cls_w, cls_out)
        if tuple(cls_w.shape) != (32, 1, 1, Cout) or cls_w.dtype != x.dtype or not cls_w.is_contiguous():
            raise ValueError(f"conv2d: cls_w must be a contiguous (32,1,1,{Cout}) packed weight of the activation dtype")
        if cls_out.dtype != torch.float32 or tuple(cls_out.shape[:3]) != (N, Ho, Wo) or cls_out.shape[3] > 32 or cls_out.stride(3) != 1:
            raise ValueError("conv2d: cls_out must be (N,Ho,Wo,ncls <= 32) fp32")
        ep.cls_w, ep.cls_out, ep.ld_cls, ep.ncls = _ptr(cls_w), _ptr(cls_out), nhwc_ld(cls_out), cls_out.shape[3]
        if x2 is not None or not _lib.lib().kd_conv2d_cls_supported(C.byref(d), C.byref(ep)):
            raise ClsUnsupported(f"conv2d: no classifier epilogue for {kh}x{kw} {H}x{W} {Cin}->{Cout}")
    sums_rows = 0
    if bn_sums is not None and mask is not None:
        sums_rows = int(_lib.lib().kd_conv2d_bn_sums_rows(C.byref(d), C.byref(ep)))
        if sums_rows > 0:
            part = _scratch((sums_rows, 2, Cout), torch.float32, x.device)
            ep.bn_sums = _ptr(part)
    out_rows = 0
    if out_sums is not None and mask is None and res_pre is None and res_post is None and out_act is None and out_raw is not None:
        out_rows = int(_lib.lib().kd_conv2d_bn_sums_rows(C.byref(d), C.byref(ep)))
        if out_rows > 0:
            opart = _scratch((out_rows, 2, Cout), torch.float32, x.device)
            ep.bn_sums = _ptr(opart)
    prof = PROFILER
    if prof is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    if x2 is not None:
        ld2 = nhwc_ld(x2)
        if not _lib.lib().kd_conv1x1_dual_supported(C.byref(d), Cin2, ld2, C.byref(ep)):
            raise DualUnsupported(f"conv2d: no K-concatenated kernel for {H}x{W} {Cin}+{Cin2}->{Cout}")
        check(_lib.lib().kd_conv1x1_dual_fwd(C.byref(d), _ptr(x), _ptr(x2), Cin2, ld2, _ptr(w_packed), C.byref(ep), stream_ptr()), "kd_conv1x1_dual_fwd")
    else:
        check(_lib.lib().kd_conv2d_fwd(C.byref(d), _ptr(x), _ptr(w_packed), C.byref(ep), stream_ptr()), "kd_conv2d_fwd")
    if out_rows > 0:
        out_sums.append(opart)      # (only once the launch was accepted: a refused one leaves the list empty)
    if prof is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        epi = "".join(c for c, t in (("p", res_pre), ("m", mask), ("q", res_post), ("r", out_raw), ("a", out_act), ("c", cls_out)) if t is not None)
        prof.append(("conv_igemm", 2.0 * N * Ho * Wo * (algo_cout or Cout) * kh * kw * (algo_cin or (Cin + Cin2)), e0, e1,
                     f"{kh}x{kw} s{stride} d{dil} {H}x{W} {Cin}{'+%d' % Cin2 if Cin2 else ''}->{Cout} [{epi}{'s' if sums_rows or out_rows else ''}]", _lib.last_kernel()))
    if sums_rows > 0:
        s12 = torch.empty((2, Cout), dtype=torch.float32, device=x.device)
        need = _lib.lib().kd_bn_sums_finish_workspace(sums_rows, Cout)
        ws = _ws(need, x.device) if need else None
        check(_lib.lib().kd_bn_sums_finish(_ptr(part), sums_rows, Cout, _ptr(s12[0]), _ptr(s12[1]), _ptr(ws), need, stream_ptr()),
              "kd_bn_sums_finish")
        bn_sums.append((s12[0], s12[1]))
    return out_raw, out_act


def conv_cls_ok(x, Cout, k=3, dil=1):
    """Does the kernel kd_conv2d_fwd selects for this 'same' conv of x carry the classifier epilogue (conv2d(..., cls_w=, cls_out=))?"""
    if not x.is_cuda or x.dtype != torch.bfloat16 or os.environ.get("KDCC_FUSE_CLS", "1") == "0":
        return False
    N, H, W, Cin = x.shape
    d = ConvDesc(dt_of(x), N, H, W, Cin, H, W, Cout, k, k, 1, dil * (k // 2), dil, nhwc_ld(x))
    ep = ConvEpilogue()
    ep.cls_w, ep.cls_out, ep.ld_cls, ep.ncls = C.c_void_p(256), C.c_void_p(256), 32, 19     # (the selection reads alignment and sizes only)
    return bool(_lib.lib().kd_conv2d_cls_supported(C.byref(d), C.byref(ep)))


def conv1x1_dual_ok(x, x2, Cout, operands=0):
    """Does the K-concatenated 1x1 kernel take [x | x2] -> Cout with `operands` epilogue operands (dense, freshly allocated outputs)?"""
    if x2 is None or not x.is_cuda or x.dtype != torch.bfloat16 or x2.dtype != x.dtype or tuple(x2.shape[:3]) != tuple(x.shape[:3]):
        return False
    N, H, W, Cin = x.shape
    d = ConvDesc(dt_of(x), N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1, nhwc_ld(x))
    ep = ConvEpilogue()
    some = C.c_void_p(x.data_ptr())          # (alignment and strides are all the selection reads of an operand)
    if operands >= 1:
        ep.mask, ep.ld_mask = some, Cout
    if operands >= 2:
        ep.res_post, ep.ld_res_post = some, Cout
    if operands >= 3:
        ep.res_pre, ep.ld_res_pre = some, Cout
    ep.out_raw, ep.ld_raw = some, Cout
    return bool(_lib.lib().kd_conv1x1_dual_supported(C.byref(d), x2.shape[3], nhwc_ld(x2), C.byref(ep)))


def conv1x1_dual_ok_dims(N, H, W, Cin, Cin2, Cout, dtype, operands=0):
    """conv1x1_dual_ok for dense tensors of these sizes (before they exist)."""
    if dtype != torch.bfloat16:
        return False
    d = ConvDesc(KD_BF16, N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1, Cin)
    ep = ConvEpilogue()
    if operands >= 1:
        ep.mask, ep.ld_mask = C.c_void_p(256), Cout       # (the selection reads only alignment and strides of an operand)
    if operands >= 2:
        ep.res_post, ep.ld_res_post = C.c_void_p(256), Cout
    if operands >= 3:
        ep.res_pre, ep.ld_res_pre = C.c_void_p(256), Cout
    ep.out_raw, ep.ld_raw = C.c_void_p(256), Cout
    return bool(_lib.lib().kd_conv1x1_dual_supported(C.byref(d), Cin2, Cin2, C.byref(ep)))


def pw_wgrad(a, dy, dw, accumulate=False, workspace=None):
    """dw (Cout,Cin,1,1) fp32 = sum_pixels dy (N,H,W,Cout) x a (N,H,W,Cin)."""
    _need_cuda(a, dy, dw)
    N, H, W, Cin = a.shape
    Cout = dy.shape[3]
    if tuple(dy.shape[:3]) != (N, H, W) or a.dtype != dy.dtype:
        raise ValueError("pw_wgrad: a / dy mismatch")
    if dw.dtype != torch.float32 or dw.numel() != Cout * Cin or not dw.is_contiguous():
        raise ValueError("pw_wgrad: dw must be contiguous fp32 (Cout,Cin,1,1)")
    M = N * H * W
    need = _lib.lib().kd_pw_wgrad_workspace(M, Cin, Cout)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = _ws(need, a.device, 0)
    e0 = _prof_start()
    check(_lib.lib().kd_pw_wgrad(dt_of(a), M, Cin, Cout, _ptr(a), nhwc_ld(a), _ptr(dy), nhwc_ld(dy), _ptr(dw),
                                 int(accumulate), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                 stream_ptr()), "kd_pw_wgrad")
    _prof_stop(e0, "pw_wgrad", 2.0 * M * Cin * Cout, f"pw wgrad {H}x{W} {Cin}->{Cout}")
    return dw


def conv2d_wgrad(x, dy, dw, stride=1, pad=0, dil=1, accumulate=False, workspace=None):
    """dw (Cout,Cin,kh,kw) fp32 = weight gradient of conv2d(x; stride, pad, dil) given dy (N,Ho,Wo,Cout)."""
    _need_cuda(x, dy, dw)
    N, H, W, Cin = x.shape
    Cout, Cin_w, kh, kw = dw.shape
    Ho, Wo = conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil)
    if Cin_w != Cin or tuple(dy.shape) != (N, Ho, Wo, Cout) or dy.dtype != x.dtype:
        raise ValueError(f"conv2d_wgrad: x {tuple(x.shape)} / dy {tuple(dy.shape)} / dw {tuple(dw.shape)} mismatch")
    if dw.dtype != torch.float32 or not dw.is_contiguous():
        raise ValueError("conv2d_wgrad: dw must be contiguous fp32 (Cout,Cin,kh,kw)")
    d = ConvDesc(dt_of(x), N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil, nhwc_ld(x))
    need = _lib.lib().kd_conv2d_wgrad_workspace(C.byref(d))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = _ws(need, x.device, 0)
    prof = PROFILER
    if prof is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    check(_lib.lib().kd_conv2d_wgrad(C.byref(d), _ptr(x), _ptr(dy), nhwc_ld(dy), _ptr(dw), int(accumulate), _ptr(workspace),
                                     workspace.numel() * workspace.element_size(), stream_ptr()), "kd_conv2d_wgrad")
    if prof is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        prof.append(("conv_wgrad", 2.0 * N * Ho * Wo * Cout * kh * kw * Cin, e0, e1,
                     f"wgrad {kh}x{kw} s{stride} d{dil} {H}x{W} {Cin}->{Cout}", _lib.last_kernel()))
    return dw


# --------------------------------------------------------------------------- depthwise conv
def pack_dw_weight(w, flip=False):
    """(C,1,k,k) fp32 -> tap-major [k*k][C] fp32 (flip=True: the dgrad operand)."""
    _need_cuda(w)
    w = w.detach().contiguous().float()
    Cc, one, k, k2 = w.shape
    if one != 1 or k != k2:
        raise ValueError("pack_dw_weight: expected (C,1,k,k)")
    out = torch.empty((k * k, Cc), dtype=torch.float32, device=w.device)
    check(_lib.lib().kd_pack_dw_weight(_ptr(w), _ptr(out), Cc, k, int(flip), stream_ptr()), "kd_pack_dw_weight")
    return out


def _dw_desc(x, k, pad, dil, y=None):
    N, H, W, Cc = x.shape
    return DwDesc(dt_of(x), N, H, W, Cc, k, pad, dil, nhwc_ld(x), nhwc_ld(y) if y is not None else Cc)


# The checks the depthwise wrappers share (`who` names the public function in the message)
def _dw_taps(who, w_taps, k, Cc):
    for w in w_taps:
        if tuple(w.shape) != (k * k, Cc) or w.dtype != torch.float32 or not w.is_contiguous():
            raise ValueError(f"{who}: w_taps must be contiguous fp32 [k*k][C]")


def _dw_grads(who, dws, k, Cc):
    for dw in dws:
        if dw.dtype != torch.float32 or dw.numel() != Cc * k * k or not dw.is_contiguous():
            raise ValueError(f"{who}: dw must be contiguous fp32 (C,1,k,k)")


def _dw_out(who, out, shape, like):
    """`out`, or a new tensor, as an NHWC view of `shape` in `like`'s dtype."""
    if out is None:
        out = torch.empty(shape, dtype=like.dtype, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype:
        raise ValueError(f"{who}: bad output view")
    return out


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[_ptr(t) for t in ts])


def _lattice_t(ts):
    return [t.t for t in ts]


def dwconv(x, w_taps, k, pad, dil, bias=None, out=None, res_pre=None, mask=None, mask_scale=None, res_post=None):
    _need_cuda(x, w_taps, bias, out, res_pre, mask, mask_scale, res_post)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        bias = bias.detach().float().contiguous()      # the kernel reads fp32 (C) (a bf16 module's parameter is not)
    N, H, W, Cc = x.shape
    _dw_taps("dwconv", [w_taps], k, Cc)
    out = _dw_out("dwconv", out, (N, H, W, Cc), x)
    d = _dw_desc(x, k, pad, dil, out)
    ep = None
    if res_pre is not None or mask is not None or res_post is not None:
        ep = DwEpilogue()
        for name, t in (("res_pre", res_pre), ("mask", mask), ("res_post", res_post)):
            if t is not None and (tuple(t.shape) != (N, H, W, Cc) or t.dtype != x.dtype):
                raise ValueError(f"dwconv: {name} must match the output shape/dtype")
            setattr(ep, name, _ptr(t))
            setattr(ep, "ld_" + name, nhwc_ld(t) if t is not None else 0)
        if mask_scale is not None and (mask_scale.dtype != torch.float32 or mask_scale.numel() != Cc):
            raise ValueError("dwconv: mask_scale must be fp32 (C,)")
        ep.mask_scale = _ptr(mask_scale)
    e0 = _prof_start()
    check(_lib.lib().kd_dwconv_fwd(C.byref(d), _ptr(x), _ptr(w_taps), _ptr(bias), C.byref(ep) if ep is not None else None,
                                   _ptr(out), stream_ptr()), "kd_dwconv_fwd")
    _prof_stop(e0, "depthwise", _nbytes(x, out, res_pre, mask, res_post), f"dw {k}x{k} d{dil} {H}x{W} C{Cc}" + (" +epi" if ep is not None else ""))
    return out


def scale_by_device_scalar_(x, scale):
    """x *= scale (0-dim / 1-element device tensor) in place; when the scalar is exactly 1 -- decided on the device, no host
    sync -- nothing is read or written.  The upstream-gradient factor of the fused loss Functions (layerwise_trainer.py:229-235)."""
    _need_cuda(x, scale)
    if scale.numel() != 1:
        raise ValueError("scale_by_device_scalar_: scale must hold one element")
    dense = x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))
    if not dense:
        x.mul_(scale.to(x.dtype))     # a strided view: plain torch
        return x
    scale = scale.detach().reshape(1)
    if scale.dtype != torch.float32:
        scale = scale.float()
    check(_lib.lib().kd_scale_by_device_scalar(_ptr(x), dt_of(x), x.numel(), _ptr(scale), stream_ptr()), "kd_scale_by_device_scalar")
    return x


def _dwconv_sum(xs, w_taps, k, pad, dil, out, lattice):
    """dwconv_sum and its lattice twin: the inputs are NHWC views, or Lattice tensors whose cells are dense (pixel stride C)."""
    who, tag = ("dwconv_sum_lattice", " [lattice]") if lattice else ("dwconv_sum", "")
    N, H, W, Cc = xs[0].shape
    _need_cuda(*(_lattice_t(xs) if lattice else xs), *w_taps, out)
    if not lattice:
        ld = nhwc_ld(xs[0])
        if any(tuple(x.shape) != (N, H, W, Cc) or x.dtype != xs[0].dtype or nhwc_ld(x) != ld for x in xs):
            raise ValueError("dwconv_sum: inputs must share shape, dtype and pixel stride")
    _dw_taps(who, w_taps, k, Cc)
    out = _dw_out(who, out, (N, H, W, Cc), xs[0])
    d = DwDesc(dt_of(out), N, H, W, Cc, k, pad, dil, Cc if lattice else nhwc_ld(xs[0]), nhwc_ld(out))
    n = len(xs)
    entry = "kd_dwconv_fwd_sum_lattice" if lattice else "kd_dwconv_fwd_sum"
    e0 = _prof_start()
    check(getattr(_lib.lib(), entry)(C.byref(d), n, _ptrs(_lattice_t(xs) if lattice else xs), _ptrs(w_taps), _ptr(out), stream_ptr()), entry)
    _prof_stop(e0, "depthwise", out.numel() * out.element_size() * (1 + n) if lattice else _nbytes(out, *xs),
               f"dw sum of {n} {k}x{k} d{dil} {H}x{W} C{Cc}{tag}")
    return out


def dwconv_sum(xs, w_taps, k, pad, dil, out=None):
    """out = sum_i dwconv(xs[i], w_taps[i]): the input gradient of a tensor that feeds several depthwise convs of one geometry
    (deeplabv3.py:64-75, the ASPP input under its replaced branches), summed inside one launch where the shape allows."""
    xs, w_taps = list(xs), list(w_taps)
    if not xs or len(xs) != len(w_taps):
        raise ValueError("dwconv_sum: need as many tap tables as inputs")
    return _dwconv_sum(xs, w_taps, k, pad, dil, out, False)


def _dwconv_fanout(x, w_taps, k, pad, dil, outs, lattice):
    """dwconv_fanout and its lattice twin: the outputs are NHWC views of one pixel stride, or Lattice tensors."""
    who, tag = ("dwconv_fanout_lattice", " [lattice]") if lattice else ("dwconv_fanout", "")
    N, H, W, Cc = x.shape
    _dw_taps(who, w_taps, k, Cc)
    if outs is None:
        outs = [Lattice(N, H, W, Cc, dil, x.dtype, x.device) if lattice else torch.empty((N, H, W, Cc), dtype=x.dtype, device=x.device) for _ in w_taps]
    outs = list(outs)
    if lattice:
        if len(outs) != len(w_taps) or any(o.shape != (N, H, W, Cc) or o.dil != dil or o.dtype != x.dtype for o in outs):
            raise ValueError("dwconv_fanout_lattice: need one matching Lattice per tap table")
    else:
        if len(outs) != len(w_taps):
            raise ValueError("dwconv_fanout: need one output per tap table")
        ld = nhwc_ld(outs[0])
        if any(tuple(o.shape) != (N, H, W, Cc) or o.dtype != x.dtype or nhwc_ld(o) != ld for o in outs):
            raise ValueError("dwconv_fanout: outputs must share shape, dtype and pixel stride")
    d = _dw_desc(x, k, pad, dil, None if lattice else outs[0])
    n = len(outs)
    entry = "kd_dwconv_fwd_fanout_lattice" if lattice else "kd_dwconv_fwd_fanout"
    e0 = _prof_start()
    check(getattr(_lib.lib(), entry)(C.byref(d), n, _ptr(x), _ptrs(w_taps), _ptrs(_lattice_t(outs) if lattice else outs), stream_ptr()), entry)
    _prof_stop(e0, "depthwise", x.numel() * x.element_size() * (1 + n) if lattice else _nbytes(x, *outs),
               f"dw fan-out of {n} {k}x{k} d{dil} {H}x{W} C{Cc}{tag}")
    return outs


def dwconv_fanout(x, w_taps, k, pad, dil, outs=None):
    """[dwconv(x, w) for w in w_taps]: several depthwise convs of one geometry reading the same tensor (deeplabv3.py:71-75,
    the ASPP branches), one pass over x where the shape allows."""
    w_taps = list(w_taps)
    if not w_taps:
        raise ValueError("dwconv_fanout: no tap tables")
    _need_cuda(x, *w_taps, *(outs or []))
    return _dwconv_fanout(x, w_taps, k, pad, dil, outs, False)


def dwconv_wgrad(x, dy, dw, k, pad, dil, accumulate=False, workspace=None):
    _need_cuda(x, dy, dw)
    N, H, W, Cc = x.shape
    if tuple(dy.shape) != (N, H, W, Cc) or dy.dtype != x.dtype:
        raise ValueError("dwconv_wgrad: x / dy mismatch")
    _dw_grads("dwconv_wgrad", [dw], k, Cc)
    d = _dw_desc(x, k, pad, dil)
    need = _lib.lib().kd_dwconv_wgrad_workspace(C.byref(d))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = _ws(need, x.device, 0)
    e0 = _prof_start()
    check(_lib.lib().kd_dwconv_wgrad(C.byref(d), _ptr(x), _ptr(dy), nhwc_ld(dy), _ptr(dw), int(accumulate), _ptr(workspace),
                                     workspace.numel() * workspace.element_size(), stream_ptr()), "kd_dwconv_wgrad")
    _prof_stop(e0, "depthwise", _nbytes(x, dy), f"dw wgrad {k}x{k} d{dil} {H}x{W} C{Cc}")
    return dw


def _dwconv_wgrad_multi(x, dys, dws, k, pad, dil, accumulate, lattice):
    """dwconv_wgrad_multi and its lattice twin, once the gradients dys (NHWC views of one pixel stride, or Lattice tensors) are checked."""
    who, tag = ("dwconv_wgrad_multi_lattice", " [lattice]") if lattice else ("dwconv_wgrad_multi", "")
    N, H, W, Cc = x.shape
    _dw_grads(who, dws, k, Cc)
    d = _dw_desc(x, k, pad, dil)
    n = len(dys)
    need = _lib.lib().kd_dwconv_wgrad_multi_workspace(C.byref(d), n)
    workspace = _ws(need, x.device)
    yp, wp = _ptrs(_lattice_t(dys) if lattice else dys), _ptrs(dws)
    e0 = _prof_start()
    if lattice:
        rc = _lib.lib().kd_dwconv_wgrad_multi_lattice(C.byref(d), n, _ptr(x), yp, wp, int(accumulate), _ptr(workspace), need, stream_ptr())
    else:
        rc = _lib.lib().kd_dwconv_wgrad_multi(C.byref(d), n, _ptr(x), yp, nhwc_ld(dys[0]), wp, int(accumulate), _ptr(workspace), need, stream_ptr())
    check(rc, "kd_" + who)
    _prof_stop(e0, "depthwise", x.numel() * x.element_size() * (1 + n) if lattice else _nbytes(x, *dys),
               f"dw wgrad of {n} {k}x{k} d{dil} {H}x{W} C{Cc}{tag}")
    return dws


def dwconv_wgrad_multi(x, dys, dws, k, pad, dil, accumulate=False):
    """dws[i] = weight gradient of dwconv(x, .) given dys[i]: several depthwise convs of one geometry reading the same tensor
    (deeplabv3.py:71-75, the replaced ASPP branches); one launch for two or three branches where the shape allows."""
    dys, dws = list(dys), list(dws)
    if not dys or len(dys) != len(dws):
        raise ValueError("dwconv_wgrad_multi: need one gradient buffer per dy")
    _need_cuda(x, *dys, *dws)
    N, H, W, Cc = x.shape
    ld = nhwc_ld(dys[0])
    if any(tuple(dy.shape) != (N, H, W, Cc) or dy.dtype != x.dtype or nhwc_ld(dy) != ld for dy in dys):
        raise ValueError("dwconv_wgrad_multi: every dy must match x's shape / dtype and share one pixel stride")
    return _dwconv_wgrad_multi(x, dys, dws, k, pad, dil, accumulate, False)


# ------------------------------------------------------------------ lattice-planar intermediates (include/kdcc.h)
class Lattice:
    """An (N,H,W,C) bf16 tensor in the lattice-planar layout of dilation `dil`: `t` is (C/16, rows, 16) -- the depthwise outputs of
    the replaced ASPP branches and their gradients, which only the depthwise kernels and the 1x1 convs next to them read
    (depthwise_separable_conv.py:11-13 under deeplabv3.py:64-75).  Not an image any more: `to_nhwc()` is for tests."""

    def __init__(self, N, H, W, Cc, dil, dtype=torch.bfloat16, device="cuda", t=None):
        self.N, self.H, self.W, self.C, self.dil = N, H, W, Cc, dil
        self.rows = lattice_rows(N, H, W, dil)
        if Cc % 16:
            raise ValueError("Lattice: channels must be a multiple of 16")
        self.t = t if t is not None else torch.empty((Cc // 16, self.rows, 16), dtype=dtype, device=device)
        if tuple(self.t.shape) != (Cc // 16, self.rows, 16) or not self.t.is_contiguous():
            raise ValueError("Lattice: bad storage")
        used = N * dil * dil * (-(-H // dil)) * (-(-W // dil))
        if t is None and used < self.rows:
            self.t[:, used:].zero_()          # the tail rows of every plane hold zeros (nobody else writes them)

    dtype = property(lambda self: self.t.dtype)
    device = property(lambda self: self.t.device)
    shape = property(lambda self: (self.N, self.H, self.W, self.C))
    plane = property(lambda self: self.rows * 16)

    def same_geometry(self, o):
        return (self.N, self.H, self.W, self.C, self.dil, self.dtype) == (o.N, o.H, o.W, o.C, o.dil, o.dtype)

    def to_nhwc(self):
        """Image-order copy (tests / debugging): plain torch indexing, not a kernel."""
        rows = self.t.permute(1, 0, 2).reshape(self.rows, self.C)
        out = torch.empty((self.N, self.H, self.W, self.C), dtype=self.dtype, device=self.device)
        return lattice_to_image(rows, out, self.dil)


def lattice_rows(N, H, W, dil):
    return int(_lib.lib().kd_lattice_rows(N, H, W, dil))


def dwconv_lattice_ok(x, n, k, pad, dil):
    """Can n (2, 3) depthwise convs of this geometry reading / summing into x-shaped tensors keep lattice-planar intermediates?"""
    if not x.is_cuda or x.dtype != torch.bfloat16:
        return False
    return bool(_lib.lib().kd_dwconv_lattice_ok(C.byref(_dw_desc(x, k, pad, dil)), n))


def image_to_lattice(img, dil, out=None):
    """(N,H,W,C) view -> dense [rows][C] in lattice row order (zero rows where a lattice cell has no pixel)."""
    _need_cuda(img, out)
    N, H, W, Cc = img.shape
    rows = lattice_rows(N, H, W, dil)
    if out is None:
        out = torch.empty((rows, Cc), dtype=img.dtype, device=img.device)
    if tuple(out.shape) != (rows, Cc) or out.dtype != img.dtype or out.stride(1) != 1:
        raise ValueError("image_to_lattice: bad output")
    e0 = _prof_start()
    check(_lib.lib().kd_lattice_rows_move(dt_of(img), N, H, W, Cc, dil, _ptr(img), nhwc_ld(img), _ptr(out), out.stride(0), 1, stream_ptr()),
          "kd_lattice_rows_move")
    _prof_stop(e0, "plumbing", _nbytes(img, out), f"rows to lattice order {H}x{W} C{Cc}")
    return out


def lattice_to_image(rows, img, dil):
    """Dense [rows][C] in lattice row order -> the (N,H,W,C) view `img`."""
    _need_cuda(img, rows)
    N, H, W, Cc = img.shape
    if tuple(rows.shape) != (lattice_rows(N, H, W, dil), Cc) or rows.dtype != img.dtype or rows.stride(1) != 1:
        raise ValueError("lattice_to_image: bad input")
    e0 = _prof_start()
    check(_lib.lib().kd_lattice_rows_move(dt_of(img), N, H, W, Cc, dil, _ptr(img), nhwc_ld(img), _ptr(rows), rows.stride(0), 0, stream_ptr()),
          "kd_lattice_rows_move")
    _prof_stop(e0, "plumbing", _nbytes(img, rows), f"rows to image order {H}x{W} C{Cc}")
    return img


def dwconv_fanout_lattice(x, w_taps, k, pad, dil, outs=None):
    """dwconv_fanout with lattice-planar outputs (n = 2, 3; dwconv_lattice_ok)."""
    w_taps = list(w_taps)
    _need_cuda(x, *w_taps)
    return _dwconv_fanout(x, w_taps, k, pad, dil, outs, True)


def dwconv_sum_lattice(xs, w_taps, k, pad, dil, out=None):
    """dwconv_sum over lattice-planar inputs (n = 2, 3); the sum is an NHWC tensor."""
    xs, w_taps = list(xs), list(w_taps)
    if len(xs) != len(w_taps) or not xs or any(not xs[0].same_geometry(x) for x in xs) or xs[0].dil != dil:
        raise ValueError("dwconv_sum_lattice: need matching Lattice inputs, one tap table each")
    return _dwconv_sum(xs, w_taps, k, pad, dil, out, True)


def dwconv_wgrad_multi_lattice(x, dys, dws, k, pad, dil, accumulate=False):
    """dwconv_wgrad_multi with lattice-planar gradients dys (n = 2, 3)."""
    dys, dws = list(dys), list(dws)
    N, H, W, Cc = x.shape
    if len(dys) != len(dws) or not dys or any(dy.shape != (N, H, W, Cc) or dy.dil != dil or dy.dtype != x.dtype for dy in dys):
        raise ValueError("dwconv_wgrad_multi_lattice: need one matching Lattice gradient per weight gradient")
    _need_cuda(x, *_lattice_t(dys), *dws)
    return _dwconv_wgrad_multi(x, dys, dws, k, pad, dil, accumulate, True)


# ------------------------------------------------------------------------------ trunk plumbing
def stem_conv(x_nchw, w, dtype):
    """(N,3,H,W) fp32 NCHW batch + (64,3,3,3) fp32 weight -> (N,H,W,64) NHWC."""
    _need_cuda(x_nchw, w)
    if x_nchw.dtype != torch.float32 or not x_nchw.is_contiguous() or x_nchw.shape[1] != 3:
        raise ValueError("stem_conv: expects a contiguous fp32 (N,3,H,W) batch")
    if tuple(w.shape) != (64, 3, 3, 3) or w.dtype != torch.float32 or not w.is_contiguous():
        raise ValueError("stem_conv: expects a contiguous fp32 (64,3,3,3) weight")
    N, _, H, W = x_nchw.shape
    y = torch.empty((N, H, W, 64), dtype=dtype, device=x_nchw.device)
    check(_lib.lib().kd_stem_conv(dt_of(y), _ptr(x_nchw), _ptr(w), _ptr(y), N, H, W, stream_ptr()), "kd_stem_conv")
    return y


def stem_conv_pool(x_nchw, w, scale=None, shift=None, want_raw=True):
    """stem conv -> pool2 (-> BN/ReLU of the consumer) in one pass, bf16, the full-resolution tensor never stored
    (wider_resnet.py:307-309, 353-356).  Returns (raw, act) like maxpool3x3s2; bit-identical to stem_conv + maxpool3x3s2."""
    _need_cuda(x_nchw, w, scale, shift)
    if x_nchw.dtype != torch.float32 or not x_nchw.is_contiguous() or x_nchw.shape[1] != 3:
        raise ValueError("stem_conv_pool: expects a contiguous fp32 (N,3,H,W) batch")
    if tuple(w.shape) != (64, 3, 3, 3) or w.dtype != torch.float32 or not w.is_contiguous():
        raise ValueError("stem_conv_pool: expects a contiguous fp32 (64,3,3,3) weight")
    N, _, H, W = x_nchw.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y_raw = torch.empty((N, Ho, Wo, 64), dtype=torch.bfloat16, device=x_nchw.device) if want_raw else None
    y_act = torch.empty((N, Ho, Wo, 64), dtype=torch.bfloat16, device=x_nchw.device) if scale is not None else None
    check(_lib.lib().kd_stem_conv_pool(_ptr(x_nchw), _ptr(w), _ptr(y_raw), _ptr(y_act), _ptr(scale), _ptr(shift), N, H, W,
                                       stream_ptr()), "kd_stem_conv_pool")
    return y_raw, y_act


def maxpool3x3s2(x, scale=None, shift=None, want_raw=True, out_raw=None, out_act=None):
    """out_raw / out_act: (N,Ho,Wo,C) views (channel slices of wider buffers) to write instead of fresh tensors."""
    _need_cuda(x, scale, shift, out_raw, out_act)
    N, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for t in (out_raw, out_act):
        if t is not None and (tuple(t.shape) != (N, Ho, Wo, Cc) or t.dtype != x.dtype):
            raise ValueError("maxpool3x3s2: bad output view")
    if out_act is not None and (scale is None or shift is None):
        raise ValueError("maxpool3x3s2: out_act needs scale and shift")
    if out_raw is not None and not want_raw:
        raise ValueError("maxpool3x3s2: out_raw given with want_raw=False")
    y_raw = out_raw if out_raw is not None else (torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device) if want_raw else None)
    y_act = out_act if out_act is not None else (torch.empty((N, Ho, Wo, Cc), dtype=x.dtype, device=x.device) if scale is not None else None)
    ld = lambda t: nhwc_ld(t) if t is not None else Cc
    check(_lib.lib().kd_maxpool3x3s2(dt_of(x), _ptr(x), nhwc_ld(x), _ptr(y_raw), ld(y_raw), _ptr(y_act), ld(y_act), _ptr(scale), _ptr(shift),
                                     N, H, W, Cc, stream_ptr()), "kd_maxpool3x3s2")
    return y_raw, y_act


def upsample_bilinear_ac(x, size, out=None, out_dtype=None, align_corners=True):
    _need_cuda(x, out)
    N, H, W, Cc = x.shape
    Ho, Wo = size
    if out is None:
        out = torch.empty((N, Ho, Wo, Cc), dtype=out_dtype or x.dtype, device=x.device)
    if tuple(out.shape) != (N, Ho, Wo, Cc):
        raise ValueError("upsample: bad output view")
    check(_lib.lib().kd_upsample_bilinear(_ptr(x), dt_of(x), nhwc_ld(x), _ptr(out), dt_of(out), nhwc_ld(out), N, H, W, Cc,
                                          Ho, Wo, int(bool(align_corners)), stream_ptr()), "kd_upsample_bilinear")
    return out


def aspp_image_pool(x, w, scale, shift, out, sums=None):
    """x (N,H,W,Cin); w (Cout,Cin[,1,1]) fp32; writes the broadcast branch into `out` (N,H,W,Cout) view.
    sums: the [N*H*W/128][2][Cin] partial rows the conv that produced x took in its epilogue (conv2d(out_sums=)): x is not read."""
    _need_cuda(x, w, scale, shift, out)
    N, H, W, Cin = x.shape
    Cout = out.shape[3]
    w = w.reshape(Cout, Cin)
    if w.dtype != torch.float32 or not w.is_contiguous() or tuple(out.shape[:3]) != (N, H, W) or out.dtype != x.dtype:
        raise ValueError("aspp_image_pool: bad operands")
    need = _lib.lib().kd_aspp_image_pool_workspace(N, Cin, Cout)
    ws = _ws(need, x.device, 0)
    if sums is not None:
        _need_cuda(sums)
        if tuple(sums.shape) != (N * H * W // 128, 2, Cin) or (H * W) % 128 or sums.dtype != torch.float32 or not sums.is_contiguous():
            raise ValueError("aspp_image_pool: sums must be the contiguous fp32 [N*H*W/128][2][Cin] partial rows of x")
        check(_lib.lib().kd_aspp_image_pool_sums(dt_of(x), _ptr(sums), _ptr(w), _ptr(scale), _ptr(shift), _ptr(out), nhwc_ld(out),
                                                 N, H, W, Cin, Cout, _ptr(ws), need, stream_ptr()), "kd_aspp_image_pool_sums")
        return out
    check(_lib.lib().kd_aspp_image_pool(dt_of(x), _ptr(x), nhwc_ld(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(out),
                                        nhwc_ld(out), N, H, W, Cin, Cout, _ptr(ws), need, stream_ptr()), "kd_aspp_image_pool")
    return out


def stem_wgrad(x_nchw, dy, dw, accumulate=False):
    """dw (64,3,3,3) fp32 from the NCHW fp32 batch and dy (N,H,W,64)."""
    _need_cuda(x_nchw, dy, dw)
    N, _, H, W = x_nchw.shape
    if x_nchw.dtype != torch.float32 or not x_nchw.is_contiguous() or x_nchw.shape[1] != 3 or tuple(dy.shape) != (N, H, W, 64):
        raise ValueError("stem_wgrad: expects a contiguous fp32 (N,3,H,W) batch and dy (N,H,W,64)")
    if tuple(dw.shape) != (64, 3, 3, 3) or dw.dtype != torch.float32 or not dw.is_contiguous():
        raise ValueError("stem_wgrad: dw must be contiguous fp32 (64,3,3,3)")
    need = _lib.lib().kd_stem_wgrad_workspace(N, H, W)
    ws = _ws(need, dy.device)
    check(_lib.lib().kd_stem_wgrad(dt_of(dy), _ptr(x_nchw), _ptr(dy), nhwc_ld(dy), _ptr(dw), N, H, W, int(accumulate), _ptr(ws), need,
                                   stream_ptr()), "kd_stem_wgrad")
    return dw


def maxpool3x3s2_bwd(x, gy, out=None, workspace=True):
    """workspace=False hands the kernel no arg-max workspace: the one-pass gather kernel runs instead of the two-pass one."""
    _need_cuda(x, gy, out)
    N, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if tuple(gy.shape) != (N, Ho, Wo, Cc) or gy.dtype != x.dtype:
        raise ValueError("maxpool3x3s2_bwd: gy must be (N,Ho,Wo,C) of the input dtype")
    if out is None:
        out = torch.empty((N, H, W, Cc), dtype=x.dtype, device=x.device)
    need = _lib.lib().kd_maxpool3x3s2_bwd_workspace(N, H, W, Cc)
    ws = _ws(need, x.device) if workspace else None
    check(_lib.lib().kd_maxpool3x3s2_bwd(dt_of(x), _ptr(x), nhwc_ld(x), _ptr(gy), nhwc_ld(gy), _ptr(out), nhwc_ld(out), N, H, W, Cc,
                                         _ptr(ws), need if workspace else 0, stream_ptr()), "kd_maxpool3x3s2_bwd")
    return out


def upsample_bilinear_ac_bwd(gy, size, out=None, out_dtype=None, align_corners=True):
    """gy (N,Ho,Wo,C) -> gradient w.r.t. the (N,H,W,C) input of upsample_bilinear_ac (same corner convention), size = (H, W)."""
    _need_cuda(gy, out)
    N, Ho, Wo, Cc = gy.shape
    H, W = size
    if out is None:
        out = torch.empty((N, H, W, Cc), dtype=out_dtype or gy.dtype, device=gy.device)
    if tuple(out.shape) != (N, H, W, Cc):
        raise ValueError("upsample_bilinear_ac_bwd: bad output view")
    need = _lib.lib().kd_upsample_bilinear_ac_bwd_workspace(N, H, W, Cc, Ho, Wo)
    ws = _ws(need, gy.device)
    check(_lib.lib().kd_upsample_bilinear_bwd(_ptr(gy), dt_of(gy), nhwc_ld(gy), _ptr(out), dt_of(out), nhwc_ld(out), N, H, W, Cc,
                                              Ho, Wo, int(bool(align_corners)), _ptr(ws), need, stream_ptr()), "kd_upsample_bilinear_bwd")
    return out


def zero_insert(x, stride, size):
    _need_cuda(x)
    N, H, W, Cc = x.shape
    Hy, Wy = size
    y = torch.empty((N, Hy, Wy, Cc), dtype=x.dtype, device=x.device)
    check(_lib.lib().kd_zero_insert(dt_of(x), _ptr(x), nhwc_ld(x), _ptr(y), Cc, N, H, W, Cc, stride, Hy, Wy, stream_ptr()),
          "kd_zero_insert")
    return y


def relu_bn_bwd(g, mask, scale, res=None, out=None):
    """(mask > 0 ? g * scale[c] : 0) + res on (N,H,W,C) views."""
    _need_cuda(g, mask, scale, res, out)
    N, H, W, Cc = g.shape
    if tuple(mask.shape) != (N, H, W, Cc) or mask.dtype != g.dtype or scale.dtype != torch.float32 or scale.numel() != Cc:
        raise ValueError("relu_bn_bwd: operand mismatch")
    if out is None:
        out = torch.empty((N, H, W, Cc), dtype=g.dtype, device=g.device)
    ldg, ldm, ldo = nhwc_ld(g), nhwc_ld(mask), nhwc_ld(out)
    check(_lib.lib().kd_relu_bn_bwd(dt_of(g), _ptr(g), ldg, _ptr(mask), ldm, _ptr(scale), _ptr(res), nhwc_ld(res) if res is not None else 0,
                                    _ptr(out), ldo, N * H * W, Cc, stream_ptr()), "kd_relu_bn_bwd")
    return out


def channel_sums(g, sub=None, a=None, per_image=False):
    """Per-channel sums over the pixels of g (N,H,W,C) [minus sub], optionally also of (g - sub) * a.
    Returns (s1, s2 | None) fp32 of shape (C,) or, with per_image, (N, C)."""
    _need_cuda(g, sub, a)
    N, H, W, Cc = g.shape
    groups, rows = (N, H * W) if per_image else (1, N * H * W)
    s1 = torch.empty((groups, Cc), dtype=torch.float32, device=g.device)
    s2 = torch.empty_like(s1) if a is not None else None
    need = _lib.lib().kd_channel_sums_workspace(groups, rows, Cc)
    ws = _ws(need, g.device)
    ld = lambda t: nhwc_ld(t) if t is not None else 0
    for t in (sub, a):
        if t is not None and (tuple(t.shape) != (N, H, W, Cc) or t.dtype != g.dtype):
            raise ValueError("channel_sums: operand mismatch")
    e0 = _prof_start()
    check(_lib.lib().kd_channel_sums(dt_of(g), _ptr(g), ld(g), _ptr(sub), ld(sub), _ptr(a), ld(a), groups, rows, Cc, _ptr(s1), _ptr(s2),
                                     _ptr(ws), need, stream_ptr()), "kd_channel_sums")
    _prof_stop(e0, "channel_sums", float(_nbytes(g, sub, a)), f"channel sums {H}x{W} C{Cc}{' -sub' if sub is not None else ''}{' *a' if a is not None else ''}",
               "channel_sums_partial_kernel")
    if not per_image:
        s1 = s1[0]
        s2 = s2[0] if s2 is not None else None
    return s1, s2


def bn_sums_finish(part):
    """part: the contiguous fp32 [rows][2][C] partial rows a conv epilogue wrote (conv2d(bn_sums=)) -> (s1, s2) fp32 (C,):
    the column sums of part[:, 0] and part[:, 1] (kd_bn_sums_finish: fp64 accumulators, fixed order)."""
    _need_cuda(part)
    if part.dim() != 3 or part.shape[1] != 2 or part.dtype != torch.float32 or not part.is_contiguous():
        raise ValueError("bn_sums_finish: part must be contiguous fp32 [rows][2][C]")
    rows, _, Cc = part.shape
    s1, s2 = torch.empty(Cc, device=part.device), torch.empty(Cc, device=part.device)
    need = _lib.lib().kd_bn_sums_finish_workspace(rows, Cc)
    ws = _ws(need, part.device)
    check(_lib.lib().kd_bn_sums_finish(_ptr(part), rows, Cc, _ptr(s1), _ptr(s2), _ptr(ws), need, stream_ptr()), "kd_bn_sums_finish")
    return s1, s2


def bn_eval_param_grads(s1, s2, scale, gamma, beta, dgamma, dbeta, accumulate=False):
    _need_cuda(s1, s2, scale, gamma, beta, dgamma, dbeta)
    Cc = s1.numel()
    for t in (s1, s2, scale, gamma, beta, dgamma, dbeta):
        if t.dtype != torch.float32 or t.numel() != Cc or not t.is_contiguous():
            raise ValueError("bn_eval_param_grads: contiguous fp32 (C,) vectors required")
    check(_lib.lib().kd_bn_eval_param_grads(_ptr(s1), _ptr(s2), _ptr(scale), _ptr(gamma), _ptr(beta), _ptr(dgamma), _ptr(dbeta), Cc,
                                            int(accumulate), stream_ptr()), "kd_bn_eval_param_grads")


def broadcast_add(v, y, alpha=1.0, accumulate=True):
    """y[n,h,w,c] (+)= alpha * v[n,c]."""
    _need_cuda(v, y)
    N, H, W, Cc = y.shape
    if tuple(v.shape) != (N, Cc) or v.dtype != torch.float32 or not v.is_contiguous():
        raise ValueError("broadcast_add: v must be contiguous fp32 (N,C)")
    check(_lib.lib().kd_broadcast_add(dt_of(y), _ptr(v), _ptr(y), nhwc_ld(y), N, H * W, Cc, C.c_float(alpha), int(accumulate),
                                      stream_ptr()), "kd_broadcast_add")
    return y


def bn_fold(bn):
    """Eval-mode nn.BatchNorm2d -> (scale, shift) fp32 device vectors."""
    g, b, m, v = bn.weight.detach().float(), bn.bias.detach().float(), bn.running_mean.float(), bn.running_var.float()
    _need_cuda(g, b, m, v)
    scale, shift = torch.empty_like(g), torch.empty_like(g)
    check(_lib.lib().kd_bn_fold(_ptr(g.contiguous()), _ptr(b.contiguous()), _ptr(m.contiguous()), _ptr(v.contiguous()),
                                C.c_float(bn.eps), _ptr(scale), _ptr(shift), g.numel(), stream_ptr()), "kd_bn_fold")
    return scale, shift


# ------------------------------------------------------------------------- small-shape path (NCHW fp32)
def _nchw32(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("small-shape kernels take contiguous fp32 device tensors (NCHW)")


def _dconv_desc(x_shape, w_shape, stride, pad, dil, groups):
    N, Cc, H, W = x_shape
    K, cg, kh, kw = w_shape
    if cg * groups != Cc:
        raise ValueError(f"direct conv: weight {tuple(w_shape)} does not match {Cc} input channels / {groups} groups")
    return DConvDesc(N, Cc, H, W, K, kh, kw, stride, pad, dil, groups), (N, K, conv_out_size(H, kh, stride, pad, dil),
                                                                         conv_out_size(W, kw, stride, pad, dil))


def conv2d_direct(x, w, bias=None, stride=1, pad=0, dil=1, groups=1):
    _nchw32(x, w, bias)
    d, oshape = _dconv_desc(x.shape, w.shape, stride, pad, dil, groups)
    y = torch.empty(oshape, dtype=torch.float32, device=x.device)
    check(_lib.lib().kd_conv2d_direct_fwd(C.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(y), stream_ptr()), "kd_conv2d_direct_fwd")
    return y


def conv2d_direct_dgrad(dy, w, x_shape, stride=1, pad=0, dil=1, groups=1):
    _nchw32(dy, w)
    d, oshape = _dconv_desc(x_shape, w.shape, stride, pad, dil, groups)
    if tuple(dy.shape) != oshape:
        raise ValueError(f"direct dgrad: dy {tuple(dy.shape)} != {oshape}")
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy.device)
    check(_lib.lib().kd_conv2d_direct_dgrad(C.byref(d), _ptr(dy), _ptr(w), _ptr(dx), stream_ptr()), "kd_conv2d_direct_dgrad")
    return dx


def conv2d_direct_wgrad(x, dy, w_shape, stride=1, pad=0, dil=1, groups=1, want_bias=False, dw=None, db=None, accumulate=False):
    """Returns (dw, db | None).  dw / db: contiguous fp32 tensors to write (+= with accumulate) instead of fresh ones."""
    _nchw32(x, dy, dw, db)
    d, oshape = _dconv_desc(x.shape, w_shape, stride, pad, dil, groups)
    if tuple(dy.shape) != oshape:
        raise ValueError(f"direct wgrad: dy {tuple(dy.shape)} != {oshape}")
    if (dw is not None and tuple(dw.shape) != tuple(w_shape)) or (db is not None and db.numel() != w_shape[0]):
        raise ValueError("direct wgrad: dw / db do not match the weight shape")
    if accumulate and (dw is None or (db is None and want_bias)):
        raise ValueError("direct wgrad: accumulate needs the tensors to add to")
    if dw is None:
        dw = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    if db is None and want_bias:
        db = torch.empty(w_shape[0], dtype=torch.float32, device=x.device)
    check(_lib.lib().kd_conv2d_direct_wgrad(C.byref(d), _ptr(x), _ptr(dy), _ptr(dw), _ptr(db), int(bool(accumulate)), stream_ptr()),
          "kd_conv2d_direct_wgrad")
    return dw, db


def bn2d_fwd(x, gamma, beta, running_mean, running_var, training, momentum, eps, relu=False):
    """Returns (y, save_mean, save_invstd); updates the running statistics in place when training."""
    _nchw32(x, gamma, beta, running_mean, running_var)
    N, Cc = x.shape[0], x.shape[1]
    HW = x.numel() // (N * Cc)
    y = torch.empty_like(x)
    mean, invstd = torch.empty(Cc, device=x.device), torch.empty(Cc, device=x.device)
    check(_lib.lib().kd_bn2d_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(running_mean),
                                 _ptr(running_var), C.c_float(momentum), C.c_float(eps), int(training), int(relu), N, Cc, HW,
                                 stream_ptr()), "kd_bn2d_fwd")
    return y, mean, invstd


def bn2d_bwd(dy, x, y, gamma, mean, invstd, training, relu=False, need_dx=True, dgamma=None, dbeta=None, accumulate=False):
    """Returns (dx | None, dgamma, dbeta).  dgamma / dbeta: contiguous fp32 (C,) vectors to write (+= with accumulate) instead
    of fresh ones."""
    _nchw32(dy, x, y, gamma, mean, invstd, dgamma, dbeta)
    N, Cc = x.shape[0], x.shape[1]
    HW = x.numel() // (N * Cc)
    dx = torch.empty_like(x) if need_dx else None
    if accumulate and (dgamma is None or dbeta is None):
        raise ValueError("bn2d_bwd: accumulate needs dgamma and dbeta to add to")
    for t in (dgamma, dbeta):
        if t is not None and t.numel() != Cc:
            raise ValueError("bn2d_bwd: dgamma / dbeta must hold one value per channel")
    dg = torch.empty(Cc, device=x.device) if dgamma is None else dgamma
    db = torch.empty(Cc, device=x.device) if dbeta is None else dbeta
    check(_lib.lib().kd_bn2d_bwd(_ptr(dy), _ptr(x), _ptr(y), _ptr(gamma), _ptr(mean), _ptr(invstd), _ptr(dx), _ptr(dg), _ptr(db),
                                 int(training), int(relu), int(bool(accumulate)), N, Cc, HW, stream_ptr()), "kd_bn2d_bwd")
    return dx, dg, db


# ------------------------------------------------------------------------- BatchNorm2d on NHWC fp32 / bf16 views (WRN path)
def _f32vec(*vs):
    for v in vs:
        if v is not None and (not v.is_cuda or v.dtype != torch.float32 or not v.is_contiguous()):
            raise ValueError("bn_nhwc: parameters / statistics must be contiguous fp32 device vectors")


def _bn_ws(M, Cc, device, lp=False):
    L = _lib.lib()
    return _ws((L.kd_bn_nhwc_lp_workspace if lp else L.kd_bn_nhwc_workspace)(M, Cc), device)


def _bn_dtype(who, x, *others):
    """fp32 or bf16, by x; every other activation operand must have x's dtype."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{who}: fp32 or bf16 only")
    for t in others:
        if t is not None and t.dtype != x.dtype:
            raise ValueError(f"{who}: operands of mixed dtype ({t.dtype} next to {x.dtype})")
    return x.dtype == torch.bfloat16


def bn_nhwc_fwd(x, gamma, beta, running_mean, running_var, training, momentum, eps, relu=False, out=None):
    """x (N,H,W,C) fp32 or bf16 view -> (y, save_mean, save_invstd); y (x's dtype) into `out` (an (N,H,W,C) view) when given.
    Train mode updates the running statistics in place (either may be None).  The parameters and statistics are fp32 either way;
    bf16 goes to kd_bn_nhwc_lp_fwd."""
    _need_cuda(x, out)
    _f32vec(gamma, beta, running_mean, running_var)
    lp = _bn_dtype("bn_nhwc_fwd", x, out)
    N, H, W, Cc = x.shape
    if gamma.numel() != Cc or beta.numel() != Cc:
        raise ValueError(f"bn_nhwc_fwd: {Cc} channels, gamma / beta of {gamma.numel()} / {beta.numel()}")
    y = torch.empty((N, H, W, Cc), dtype=x.dtype, device=x.device) if out is None else out
    if tuple(y.shape) != (N, H, W, Cc):
        raise ValueError("bn_nhwc_fwd: out must be a view of the input's shape and dtype")
    mean, invstd = torch.empty(Cc, device=x.device), torch.empty(Cc, device=x.device)
    M = N * H * W
    ws = _bn_ws(M, Cc, x.device, lp) if training else None
    fn, name = (_lib.lib().kd_bn_nhwc_lp_fwd, "kd_bn_nhwc_lp_fwd") if lp else (_lib.lib().kd_bn_nhwc_fwd, "kd_bn_nhwc_fwd")
    check(fn(_ptr(x), nhwc_ld(x), _ptr(y), nhwc_ld(y), M, Cc, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd),
             _ptr(running_mean), _ptr(running_var), C.c_float(momentum), C.c_float(eps), int(bool(training)),
             int(bool(relu)), _ptr(ws), 0 if ws is None else ws.numel(), stream_ptr()), name)
    if training:    # the kernel updated the running statistics through raw pointers: tell version-keyed caches (BN folds)
        for t in (running_mean, running_var):
            if t is not None:
                torch.autograd.graph.increment_version(t)
    if out is not None:
        torch.autograd.graph.increment_version(out)
    return y, mean, invstd


def bn_nhwc_bwd(gy, x, y, gamma, mean, invstd, training, relu=False, res=None, need_dx=True, dgamma=None, dbeta=None,
                accumulate=False, out=None):
    """Returns dx (N,H,W,C) | None; dgamma / dbeta (contiguous fp32 (C,)) receive sum g' xhat / sum g' when given (+= with
    accumulate).  res: a gradient view added to dx.  y (the forward output) is read only with relu.
    gy, x, y, res and out are all fp32 or all bf16 (kd_bn_nhwc_lp_bwd), dx in that dtype; the per-channel vectors are fp32.
    out: an (N,H,W,C) view (a channel prefix of a wider buffer) that receives dx instead of a fresh tensor.  `out` MAY
    alias `res` exactly (same base pointer and strides: dx accumulates in place into the gradient it is added to): the dx
    kernel computes element (m, c) in one thread, which loads res[m][c] before it stores dx[m][c] and touches no other element
    of either, and the reductions that precede it read neither.  Any other overlap of `out` with an operand is refused."""
    _need_cuda(gy, x, y, res, out)
    _f32vec(gamma, mean, invstd, dgamma, dbeta)
    lp = _bn_dtype("bn_nhwc_bwd", x, gy, y, res, out)
    es = x.element_size()
    N, H, W, Cc = x.shape
    for t in (gy, y, res, out):
        if t is not None and tuple(t.shape) != (N, H, W, Cc):
            raise ValueError("bn_nhwc_bwd: operand mismatch")
    M = N * H * W
    if out is not None:
        if not need_dx:
            raise ValueError("bn_nhwc_bwd: out given with need_dx=False")
        lo, hi = out.data_ptr(), out.data_ptr() + es * ((M - 1) * nhwc_ld(out) + Cc)
        for t in (gy, x, y if relu else None, res):
            if t is None or (t is res and t.data_ptr() == lo and t.stride() == out.stride()):
                continue
            if t.data_ptr() < hi and lo < t.data_ptr() + es * ((M - 1) * nhwc_ld(t) + Cc):
                raise ValueError("bn_nhwc_bwd: out overlaps an operand (only an exact alias of res is allowed)")
        dx = out
    else:
        dx = torch.empty((N, H, W, Cc), dtype=x.dtype, device=x.device) if need_dx else None
    ws = _bn_ws(M, Cc, x.device, lp) if ((need_dx and training) or dgamma is not None or dbeta is not None) else None
    ld = lambda t: nhwc_ld(t) if t is not None else 0
    fn, name = (_lib.lib().kd_bn_nhwc_lp_bwd, "kd_bn_nhwc_lp_bwd") if lp else (_lib.lib().kd_bn_nhwc_bwd, "kd_bn_nhwc_bwd")
    check(fn(_ptr(gy), ld(gy), _ptr(x), ld(x), _ptr(y if relu else None), ld(y) if relu else 0, _ptr(res), ld(res),
             _ptr(dx), ld(dx), M, Cc, _ptr(gamma), _ptr(mean), _ptr(invstd), _ptr(dgamma), _ptr(dbeta),
             int(bool(accumulate)), int(bool(training)), int(bool(relu)), _ptr(ws),
             0 if ws is None else ws.numel(), stream_ptr()), name)
    if out is not None:
        torch.autograd.graph.increment_version(out)
    return dx


# ------------------------------------------------------------------------- DenseNet path (csrc/dense_ops.hip)
def bn_nhwc_stats(x, eps, mean=None, invstd=None, var_unbiased=None):
    """Train-mode batch statistics of an (N,H,W,C) fp32 view -> (mean, invstd, var_unbiased), each a contiguous fp32 (C,) vector
    (written into the given ones: slices of a dense block's per-channel vectors).  Per channel the bits kd_bn_nhwc_fwd saves."""
    _need_cuda(x)
    if x.dtype != torch.float32:
        raise TypeError("bn_nhwc_stats: fp32 only")
    N, H, W, Cc = x.shape
    new = lambda v: torch.empty(Cc, device=x.device) if v is None else v
    mean, invstd, var_unbiased = new(mean), new(invstd), new(var_unbiased)
    _f32vec(mean, invstd, var_unbiased)
    if not (mean.numel() == invstd.numel() == var_unbiased.numel() == Cc):
        raise ValueError(f"bn_nhwc_stats: {Cc} channels need vectors of {Cc}")
    M = N * H * W
    ws = _bn_ws(M, Cc, x.device)
    check(_lib.lib().kd_bn_nhwc_stats(_ptr(x), nhwc_ld(x), M, Cc, _ptr(mean), _ptr(invstd), _ptr(var_unbiased), C.c_float(eps), _ptr(ws),
                                      ws.numel(), stream_ptr()), "kd_bn_nhwc_stats")
    return mean, invstd, var_unbiased


def bn_nhwc_apply(x, gamma, beta, mean, invstd, var_unbiased, running_mean, running_var, momentum, relu=False, out=None):
    """Train-mode BatchNorm with supplied batch statistics (bn_nhwc_stats), one pass: y = relu?((x - mean) gamma invstd + beta),
    into `out` when given; the running statistics (either may be None) are updated in place as bn_nhwc_fwd would."""
    _need_cuda(x, out)
    _f32vec(gamma, beta, mean, invstd, var_unbiased, running_mean, running_var)
    if x.dtype != torch.float32:
        raise TypeError("bn_nhwc_apply: fp32 only")
    N, H, W, Cc = x.shape
    for v in (gamma, beta, mean, invstd, var_unbiased, running_mean, running_var):
        if v is not None and v.numel() != Cc:
            raise ValueError(f"bn_nhwc_apply: {Cc} channels, a vector of {v.numel()}")
    if running_var is not None and var_unbiased is None:
        raise ValueError("bn_nhwc_apply: running_var needs var_unbiased")
    y = torch.empty((N, H, W, Cc), dtype=torch.float32, device=x.device) if out is None else out
    if tuple(y.shape) != (N, H, W, Cc) or y.dtype != torch.float32:
        raise ValueError("bn_nhwc_apply: out must be an fp32 view of the input's shape")
    check(_lib.lib().kd_bn_nhwc_apply(_ptr(x), nhwc_ld(x), _ptr(y), nhwc_ld(y), N * H * W, Cc, _ptr(gamma), _ptr(beta), _ptr(mean),
                                      _ptr(invstd), _ptr(var_unbiased), _ptr(running_mean), _ptr(running_var), C.c_float(momentum),
                                      int(bool(relu)), stream_ptr()), "kd_bn_nhwc_apply")
    for t in (running_mean, running_var, out):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    return y


def _pool_views(x, other, shape, who):
    _need_cuda(x, other)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise TypeError(f"{who}: (N,H,W,C) fp32 views only")
    if other is not None and (tuple(other.shape) != shape or other.dtype != torch.float32):
        raise ValueError(f"{who}: out must be an fp32 {shape} view")
    return torch.empty(shape, dtype=torch.float32, device=x.device) if other is None else other


def avgpool2x2(x, out=None):
    """AvgPool2d(2, 2) of an (N,H,W,C) fp32 view -> (N, H//2, W//2, C) (an odd last row / column is dropped)."""
    N, H, W, Cc = x.shape
    y = _pool_views(x, out, (N, H // 2, W // 2, Cc), "avgpool2x2")
    check(_lib.lib().kd_avgpool2x2_nhwc(_ptr(x), nhwc_ld(x), _ptr(y), nhwc_ld(y), N, H, W, Cc, stream_ptr()), "kd_avgpool2x2_nhwc")
    return y


def avgpool2x2_bwd(gy, size, out=None):
    """gy (N, H//2, W//2, C) -> the gradient (N,H,W,C) of avgpool2x2's input, size = (H, W); dropped rows / columns get 0."""
    N, Ho, Wo, Cc = gy.shape
    H, W = size
    if (Ho, Wo) != (H // 2, W // 2):
        raise ValueError(f"avgpool2x2_bwd: gy {tuple(gy.shape)} is not the pooled size of {H}x{W}")
    gx = _pool_views(gy, out, (N, H, W, Cc), "avgpool2x2_bwd")
    check(_lib.lib().kd_avgpool2x2_nhwc_bwd(_ptr(gy), nhwc_ld(gy), _ptr(gx), nhwc_ld(gx), N, H, W, Cc, stream_ptr()),
          "kd_avgpool2x2_nhwc_bwd")
    return gx


# ------------------------------------------------------------------------- PreResNet classifier head (csrc/head_ops.hip)
def _head_operands(who, x, vecs):
    _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise TypeError(f"{who}: an (N,H,W,C) fp32 view only")
    _f32vec(*vecs)
    N, H, W, Cc = x.shape
    for v in vecs:
        if v is not None and v.numel() != Cc:
            raise ValueError(f"{who}: {Cc} channels, a vector of {v.numel()}")
    return N, H * W, Cc


def head_bn_relu_pool_fwd(x, gamma, beta, mean, invstd, var_unbiased=None, running_mean=None, running_var=None, momentum=0.0):
    """mean over the map of relu((x - mean) invstd gamma + beta) for an (N,H,W,C) fp32 view -> (N,C); the activation is never stored.
    mean / invstd: the running statistics (eval) or bn_nhwc_stats' (train); running_mean / running_var, when given, are updated
    in place from mean / var_unbiased as bn_nhwc_apply does."""
    N, HW, Cc = _head_operands("head_bn_relu_pool_fwd", x, (gamma, beta, mean, invstd, var_unbiased, running_mean, running_var))
    if running_var is not None and var_unbiased is None:
        raise ValueError("head_bn_relu_pool_fwd: running_var needs var_unbiased")
    pooled = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    check(_lib.lib().kd_head_bn_relu_pool_fwd(_ptr(x), nhwc_ld(x), N, HW, Cc, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(pooled),
                                              _ptr(var_unbiased), _ptr(running_mean), _ptr(running_var), C.c_float(momentum), stream_ptr()),
          "kd_head_bn_relu_pool_fwd")
    for t in (running_mean, running_var):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    return pooled


def head_bn_relu_pool_bwd(x, gpooled, gamma, beta, mean, invstd, training, need_dx=True, out=None):
    """Backward of head_bn_relu_pool_fwd from x itself -> (dx | None, dgamma, dbeta); gpooled a contiguous fp32 (N,C); out, an
    (N,H,W,C) fp32 view that does not overlap x, receives dx instead of a fresh tensor."""
    N, HW, Cc = _head_operands("head_bn_relu_pool_bwd", x, (gamma, beta, mean, invstd))
    _need_cuda(gpooled, out)
    if gpooled.dtype != torch.float32 or tuple(gpooled.shape) != (N, Cc) or not gpooled.is_contiguous():
        raise ValueError(f"head_bn_relu_pool_bwd: gpooled must be a contiguous fp32 ({N},{Cc}) tensor")
    if out is not None:
        if not need_dx or out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape):
            raise ValueError("head_bn_relu_pool_bwd: out must be an fp32 view of x's shape, given with need_dx only")
        M = N * HW
        lo, hi = out.data_ptr(), out.data_ptr() + 4 * ((M - 1) * nhwc_ld(out) + Cc)
        if x.data_ptr() < hi and lo < x.data_ptr() + 4 * ((M - 1) * nhwc_ld(x) + Cc):
            raise ValueError("head_bn_relu_pool_bwd: out overlaps x")
    dx = out if out is not None else (torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device) if need_dx else None)
    dgamma, dbeta = torch.empty(Cc, device=x.device), torch.empty(Cc, device=x.device)
    check(_lib.lib().kd_head_bn_relu_pool_bwd(_ptr(x), nhwc_ld(x), _ptr(gpooled), N, HW, Cc, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd),
                                              _ptr(dx), 0 if dx is None else nhwc_ld(dx), _ptr(dgamma), _ptr(dbeta), int(bool(training)),
                                              stream_ptr()), "kd_head_bn_relu_pool_bwd")
    if out is not None:
        torch.autograd.graph.increment_version(out)
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------- dropout (csrc/dropout.hip)
def dropout_params(p):
    """(threshold, scale) of a rate p in [0, 1): an element is kept iff its 32-bit random word is >= threshold = floor(p 2^32),
    kept values are multiplied by scale = float32(1 / (1 - p)).  Computed here, so the kernel is a pure function of its arguments."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout: p = {p} is outside [0, 1)")
    return int(p * 4294967296.0), C.c_float(1.0 / (1.0 - p)).value


def dropout_nhwc(x, p, seed, offset, out=None):
    """y = keep ? x / (1 - p) : 0 for an (N,H,W,C) fp32 or bf16 view (any pixel stride >= C) -- kd_dropout_nhwc.  The mask is the
    counter-based rule of csrc/dropout_rng.h: a pure function of (seed, offset, m * C + c), whatever the layout, the dtype or the
    kernel that runs, so the same call on the output gradient with the forward's (seed, offset) is the backward.  out: a view of
    x's shape and dtype that receives y (x itself for an in-place pass, otherwise one that shares no element with x); channels past C
    of a padded buffer are left alone."""
    threshold, scale = dropout_params(p)
    _need_cuda(x, out)
    if x.dim() != 4:
        raise ValueError(f"dropout_nhwc: expected an (N,H,W,C) view, got shape {tuple(x.shape)}")
    dt = dt_of(x)
    seed, offset = int(seed), int(offset)
    if not (0 <= seed < 1 << 64 and 0 <= offset < 1 << 64):
        raise ValueError("dropout_nhwc: seed and offset are unsigned 64-bit integers")
    y = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device) if out is None else out
    if tuple(y.shape) != tuple(x.shape) or y.dtype != x.dtype:
        raise ValueError("dropout_nhwc: out must be a view of the input's shape and dtype")
    N, H, W, Cc = x.shape
    if N * H * W * Cc:
        check(_lib.lib().kd_dropout_nhwc(_ptr(x), nhwc_ld(x), _ptr(y), nhwc_ld(y), dt, N * H * W, Cc, threshold, C.c_float(scale), seed, offset,
                                         stream_ptr()), "kd_dropout_nhwc")
    if out is not None and out.data_ptr() == x.data_ptr():      # in place: x changed under whoever saved it.  (A separate out is a
        torch.autograd.graph.increment_version(out)             # fresh slice of its buffer, as conv2d's out_raw and copy_cast's dst.)
    return y


# ------------------------------------------------------------------------- VGG's BN -> ReLU -> MaxPool2d(2, 2) (csrc/pool_ops.hip)
def _pool_operands(who, x, vecs):
    N, _, Cc = _head_operands(who, x, vecs)
    H, W = x.shape[1], x.shape[2]
    bn = vecs[:4]
    if any(v is None for v in bn) and any(v is not None for v in vecs):
        raise ValueError(f"{who}: gamma, beta, mean and invstd come together (all None: no BatchNorm)")
    return N, H, W, Cc


def _no_overlap(who, out, x):
    span = lambda t: (t.data_ptr(), t.data_ptr() + 4 * ((t.shape[0] * t.shape[1] * t.shape[2] - 1) * nhwc_ld(t) + t.shape[3]))
    (lo, hi), (xl, xh) = span(out), span(x)
    if xl < hi and lo < xh:
        raise ValueError(f"{who}: out overlaps x")


def bn_relu_maxpool2x2_fwd(x, gamma=None, beta=None, mean=None, invstd=None, var_unbiased=None, running_mean=None, running_var=None,
                           momentum=0.0, out=None):
    """max over every 2x2 window of relu((x - mean) (gamma invstd) + beta) for an (N,H,W,C) fp32 view -> (N,H//2,W//2,C) (into `out`, a
    view of that shape, when given); the full-resolution activation is never stored.  gamma = beta = mean = invstd = None: max(relu(x)).
    mean / invstd: the running statistics (eval) or bn_nhwc_stats' (train); running_mean / running_var, when given, are updated in
    place from mean / var_unbiased as bn_nhwc_apply does."""
    who = "bn_relu_maxpool2x2_fwd"
    N, H, W, Cc = _pool_operands(who, x, (gamma, beta, mean, invstd, var_unbiased, running_mean, running_var))
    if running_var is not None and var_unbiased is None:
        raise ValueError(f"{who}: running_var needs var_unbiased")
    shape = (N, H // 2, W // 2, Cc)
    if out is not None:
        _need_cuda(out)
        if out.dtype != torch.float32 or tuple(out.shape) != shape:
            raise ValueError(f"{who}: out must be an fp32 view of shape {shape}")
        if out.numel():
            _no_overlap(who, out, x)
    y = out if out is not None else torch.empty(shape, dtype=torch.float32, device=x.device)
    check(_lib.lib().kd_bn_relu_maxpool2x2_fwd(_ptr(x), nhwc_ld(x), N, H, W, Cc, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(y),
                                               nhwc_ld(y) if y.numel() else Cc, _ptr(var_unbiased), _ptr(running_mean), _ptr(running_var),
                                               C.c_float(momentum), stream_ptr()), "kd_bn_relu_maxpool2x2_fwd")
    for t in (running_mean, running_var, out):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    return y


def bn_relu_maxpool2x2_bwd(x, gpooled, gamma=None, beta=None, mean=None, invstd=None, training=False, need_dx=True, out=None):
    """Backward of bn_relu_maxpool2x2_fwd from x itself -> (dx | None, dgamma, dbeta) (dgamma = dbeta = None without BatchNorm): the
    pooled gradient gpooled, an (N,H//2,W//2,C) fp32 view, goes to the first maximum of every window where it is positive; nothing was
    saved by the forward.  out, an (N,H,W,C) fp32 view that does not overlap x, receives dx instead of a fresh tensor."""
    who = "bn_relu_maxpool2x2_bwd"
    N, H, W, Cc = _pool_operands(who, x, (gamma, beta, mean, invstd))
    _need_cuda(gpooled, out)
    if gpooled.dtype != torch.float32 or tuple(gpooled.shape) != (N, H // 2, W // 2, Cc):
        raise ValueError(f"{who}: gpooled must be an fp32 ({N},{H // 2},{W // 2},{Cc}) view")
    if gamma is None and not need_dx:
        raise ValueError(f"{who}: nothing requested")
    if out is not None:
        if not need_dx or out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape):
            raise ValueError(f"{who}: out must be an fp32 view of x's shape, given with need_dx only")
        _no_overlap(who, out, x)
    dx = out if out is not None else (torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device) if need_dx else None)
    dgamma = dbeta = ws = None
    if gamma is not None:
        dgamma, dbeta = torch.empty(Cc, device=x.device), torch.empty(Cc, device=x.device)
        ws = _bn_ws(N * H * W, Cc, x.device)
    check(_lib.lib().kd_bn_relu_maxpool2x2_bwd(_ptr(x), nhwc_ld(x), _ptr(gpooled), nhwc_ld(gpooled) if gpooled.numel() else Cc, N, H, W, Cc,
                                               _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(dx), 0 if dx is None else nhwc_ld(dx),
                                               _ptr(dgamma), _ptr(dbeta), int(bool(training)), _ptr(ws), 0 if ws is None else ws.numel(),
                                               stream_ptr()), "kd_bn_relu_maxpool2x2_bwd")
    if out is not None:
        torch.autograd.graph.increment_version(out)
    return dx, dgamma, dbeta


def copy_cast(src, dst):
    """dst = src for two (N,C,H,W)-logical fp32/bf16 device tensors of the same shape with any dense-plane layout
    (NCHW <-> channels_last, a channel slice of a wider NHWC buffer) -- kd_copy_cast."""
    _need_cuda(src, dst)
    if src.shape != dst.shape or src.dim() != 4:
        raise ValueError("copy_cast: shape mismatch")
    N, Cc, H, W = src.shape

    def strides(t):
        sN, sC, sH, sW = t.stride()
        if H > 1 and sH != W * sW:
            raise ValueError(f"copy_cast: rows of {tuple(t.shape)} stride {t.stride()} are not one plane")
        return sN, sC, sW
    (a, b, c), (d, e, f) = strides(src), strides(dst)
    check(_lib.lib().kd_copy_cast(_ptr(src), dt_of(src), a, b, c, _ptr(dst), dt_of(dst), d, e, f, N, Cc, H * W, stream_ptr()),
          "kd_copy_cast")
    return dst


# ------------------------------------------------------------------------- Gated-SCNN shape stream
def pointwise_small(x, w, bias=None, out=None):
    """1x1 conv + bias, bf16, (Cin, Cout) in {(64, 32), (32, 16), (16, 8)}: x (N,H,W,Cin) view, w fp32 (Cout,Cin[,1,1]) (gscnn.py:232-235)."""
    _need_cuda(x, w, bias, out)
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    w = w.detach().reshape(Cout, -1)
    if x.dtype != torch.bfloat16 or w.shape[1] != Cin or w.dtype != torch.float32 or not w.is_contiguous():
        raise ValueError("pointwise_small: bf16 (N,H,W,Cin) input and a contiguous fp32 (Cout,Cin) weight required")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != Cout or not bias.is_contiguous()):
        raise ValueError("pointwise_small: bias must be contiguous fp32 (Cout,)")
    if out is None:
        out = torch.empty((N, H, W, Cout), dtype=x.dtype, device=x.device)
    if tuple(out.shape) != (N, H, W, Cout) or out.dtype != x.dtype:
        raise ValueError("pointwise_small: bad output view")
    check(_lib.lib().kd_pointwise_small(_ptr(x), nhwc_ld(x), _ptr(w), _ptr(bias), _ptr(out), nhwc_ld(out), N * H * W, Cin, Cout,
                                        stream_ptr()), "kd_pointwise_small")
    return out


def conv3x3_small(x, w_packed, bias=None, res=None, relu=True, out=None):
    """3x3 / stride 1 / pad 1 conv on 16, 32 or 64 channels (bf16): x (N,H,W,C) view, w_packed (C,3,3,C) bf16, bias fp32 (C),
    res (N,H,W,C) view added before the ReLU (Resnet.py:64-99 BasicBlock)."""
    _need_cuda(x, w_packed, bias, res, out)
    N, H, W, Cc = x.shape
    if x.dtype != torch.bfloat16 or tuple(w_packed.shape) != (Cc, 3, 3, Cc) or w_packed.dtype != torch.bfloat16 or not w_packed.is_contiguous():
        raise ValueError("conv3x3_small: bf16 (N,H,W,C) input and a contiguous bf16 (C,3,3,C) packed weight required")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != Cc or not bias.is_contiguous()):
        raise ValueError("conv3x3_small: bias must be contiguous fp32 (C,)")
    if res is not None and (tuple(res.shape) != (N, H, W, Cc) or res.dtype != x.dtype):
        raise ValueError("conv3x3_small: res must match the output shape/dtype")
    if out is None:
        out = torch.empty((N, H, W, Cc), dtype=x.dtype, device=x.device)
    if tuple(out.shape) != (N, H, W, Cc) or out.dtype != x.dtype:
        raise ValueError("conv3x3_small: bad output view")
    check(_lib.lib().kd_conv3x3_small(_ptr(x), nhwc_ld(x), _ptr(w_packed), _ptr(bias), _ptr(res), nhwc_ld(res) if res is not None else 0,
                                      _ptr(out), nhwc_ld(out), N, H, W, Cc, int(bool(relu)), stream_ptr()), "kd_conv3x3_small")
    return out


def gated_conv(feat, gate, params, C_, out=None):
    """feat (N,H,W,>=C) view whose first C channels are the features; gate (N,H,W,1); params: packed fp32 vector
    (W1, b1, w2, b2, Wg with the BNs folded); out: (N,H,W,C) view."""
    _need_cuda(feat, gate, params, out)
    N, H, W, _ = feat.shape
    f = feat[..., :C_]
    if out is None:
        out = torch.empty((N, H, W, C_), dtype=feat.dtype, device=feat.device)
    need = (C_ + 1) * (C_ + 1) + 2 * (C_ + 1) + 1 + C_ * C_
    if params.dtype != torch.float32 or params.numel() != need or not params.is_contiguous() or gate.dtype != feat.dtype:
        raise ValueError("gated_conv: bad parameter vector / gate dtype")
    check(_lib.lib().kd_gated_conv(dt_of(feat), _ptr(f), nhwc_ld(f), _ptr(gate), gate.stride(2), _ptr(params), _ptr(out), nhwc_ld(out),
                                   N * H * W, C_, stream_ptr()), "kd_gated_conv")
    return out


def edge_attention(cs, canny, weights):
    """cs (N,H,W,>=8) view, canny (N,H,W) fp32 0/255, weights fp32 (10,) = fuse[8] + cw[2] -> acts (N,H,W) fp32."""
    _need_cuda(cs, canny, weights)
    N, H, W, _ = cs.shape
    c8 = cs[..., :8]
    acts = torch.empty((N, H, W), dtype=torch.float32, device=cs.device)
    if canny.dtype != torch.float32 or not canny.is_contiguous() or tuple(canny.shape) != (N, H, W) or weights.numel() != 10:
        raise ValueError("edge_attention: bad operands")
    check(_lib.lib().kd_edge_attention(dt_of(cs), _ptr(c8), nhwc_ld(c8), _ptr(canny), _ptr(weights), _ptr(acts), N * H * W, stream_ptr()),
          "kd_edge_attention")
    return acts


def edge_aspp(acts, w, scale, shift, out):
    """acts (N,H,W) fp32 -> out (N,Ho,Wo,C) slice: relu(bilinear(acts) * w[c] * scale[c] + shift[c])."""
    _need_cuda(acts, w, scale, shift, out)
    N, H, W = acts.shape
    _, Ho, Wo, Cc = out.shape
    check(_lib.lib().kd_edge_aspp(dt_of(out), _ptr(acts), H, W, _ptr(w), _ptr(scale), _ptr(shift), _ptr(out), nhwc_ld(out), N, Ho, Wo, Cc,
                                  stream_ptr()), "kd_edge_aspp")
    return out


def canny(x_nchw, low=10, high=100, sweeps=8, max_rounds=None, return_rounds=False):
    """Device Canny of the uint8-cast batch (N,3,H,W) -> (N,H,W) fp32 0/255.  Hysteresis runs `sweeps` sweeps per round and
    reads one device int between rounds (the reference round-trips the whole image through the host here) until a round's
    last sweep promotes nothing: the result is the hysteresis fixed point, never a partial map.  max_rounds bounds the rounds
    (the first included) and raises when it is reached without convergence; its default, ceil(H*W / sweeps) + 1, cannot bind:
    every sweep but the last promotes at least one pixel of the image that converges last.  return_rounds: -> (map, rounds)."""
    _need_cuda(x_nchw)
    if x_nchw.dtype != torch.float32 or not x_nchw.is_contiguous() or x_nchw.shape[1] != 3:
        raise ValueError("canny: expects a contiguous fp32 (N,3,H,W) batch")
    N, _, H, W = x_nchw.shape
    if sweeps < 1:
        raise ValueError("canny: sweeps must be at least 1")
    if max_rounds is None:
        max_rounds = -(-H * W // sweeps) + 1
    out = torch.empty((N, H, W), dtype=torch.float32, device=x_nchw.device)
    changed = torch.zeros(1, dtype=torch.int32, device=x_nchw.device)
    need = _lib.lib().kd_canny_workspace(N, H, W)
    ws = _ws(need, x_nchw.device)
    check(_lib.lib().kd_canny(_ptr(x_nchw), N, H, W, low, high, sweeps, _ptr(out), _ptr(changed), _ptr(ws), need, stream_ptr()), "kd_canny")
    rounds = 1
    while int(changed.item()) != 0:
        if rounds >= max_rounds:
            raise _lib.KdccError(f"canny: hysteresis of the {N} x {H} x {W} batch has not converged after {rounds} rounds "
                                 f"({rounds * sweeps} sweeps)")
        check(_lib.lib().kd_canny_continue(N, H, W, sweeps, _ptr(out), _ptr(changed), _ptr(ws), need, stream_ptr()), "kd_canny_continue")
        rounds += 1
    return (out, rounds) if return_rounds else out


# ------------------------------------------------------------------------- Gated-SCNN shape stream, backward pieces
def _rows(t):
    """(..., C) tensor with dense channels and uniformly strided pixels -> (pixel stride, pixels, channels)."""
    if t.stride(-1) != 1:
        raise ValueError("expected dense channels")
    Cc = t.shape[-1]
    npix = t.numel() // Cc
    ld = t.stride(-2) if t.dim() > 1 else Cc
    lead = t.shape[:-1]
    exp = ld
    for n, st in zip(reversed(lead), reversed(t.stride()[:-1])):   # every leading dimension must continue the pixel stride
        if n > 1 and st != exp:
            raise ValueError(f"not a pixel-strided view: shape {tuple(t.shape)} stride {t.stride()}")
        exp *= n
    return ld, npix, Cc


def small_linear(x, w, bias=None, out=None, out_dtype=None, accumulate=False, relu=False, mask=None):
    """out[p][co] (+)= bias[co] + sum_ci w[co][ci] x[p][ci]; x (..., Cin), w fp32 (Cout, Cin), <= 72 channels on either side.
    mask: fp32 (..., Cout), the result is zeroed where mask <= 0 (backward through the ReLU that produced `mask`)."""
    _need_cuda(x, w, bias, out, mask)
    ldx, npix, Cin = _rows(x)
    w = w.detach().float().contiguous()
    Cout = w.shape[0]
    if w.dim() != 2 or w.shape[1] != Cin:
        raise ValueError(f"small_linear: w {tuple(w.shape)} does not match {Cin} input channels")
    if bias is not None:
        bias = bias.detach().float().contiguous()
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (Cout,), dtype=out_dtype or x.dtype, device=x.device)
    ldy, npo, Co = _rows(out)
    if npo != npix or Co != Cout:
        raise ValueError("small_linear: bad output view")
    ldm = 0
    if mask is not None:
        ldm, npm, Cm = _rows(mask)
        if mask.dtype != torch.float32 or npm != npix or Cm != Cout:
            raise ValueError("small_linear: mask must be fp32 and match the output")
    check(_lib.lib().kd_small_linear(_ptr(x), dt_of(x), ldx, Cin, _ptr(w), _ptr(bias), _ptr(out), dt_of(out), ldy, Cout, npix, int(accumulate),
                                     int(relu), _ptr(mask), ldm, stream_ptr()), "kd_small_linear")
    return out


def small_wgrad(a, b, want_bias=False, dw=None, db=None, accumulate=False):
    """dw[cb][ca] = sum_p b[p][cb] a[p][ca] (fp32 (Cb, Ca)), db[cb] = sum_p b[p][cb]; a (..., Ca), b (..., Cb), <= 72 channels."""
    _need_cuda(a, b, dw, db)
    lda, npix, Ca = _rows(a)
    ldb, npb, Cb = _rows(b)
    if npb != npix:
        raise ValueError("small_wgrad: a and b must cover the same pixels")
    if dw is None:
        dw = torch.empty((Cb, Ca), dtype=torch.float32, device=a.device)
    if want_bias and db is None:
        db = torch.empty((Cb,), dtype=torch.float32, device=a.device)
    need = _lib.lib().kd_small_wgrad_workspace(Ca, Cb, npix)
    ws = _ws(need, a.device)
    check(_lib.lib().kd_small_wgrad(_ptr(a), dt_of(a), lda, Ca, _ptr(b), dt_of(b), ldb, Cb, npix, _ptr(dw), _ptr(db), int(accumulate), _ptr(ws),
                                    need, stream_ptr()), "kd_small_wgrad")
    return dw, db


def gate_mix_bwd(feat, a, gv=None, want_v=False):
    """GatedSpatialConv2d's tail: returns (gfeat, ga, v) -- gfeat = gv (sigmoid(a) + 1), ga = (sum_c gv feat) sigmoid'(a) (both None
    without gv), v = feat (sigmoid(a) + 1) (if want_v); fp32 outputs."""
    _need_cuda(feat, a, gv)
    ldf, npix, Cc = _rows(feat)
    if a.dtype != torch.float32 or a.numel() != npix or not a.is_contiguous():
        raise ValueError("gate_mix_bwd: a must be a contiguous fp32 tensor with one value per pixel")
    gfeat = ga = v = None
    ldgv = 0
    if gv is not None:
        if gv.dtype != torch.float32:
            raise ValueError("gate_mix_bwd: gv must be fp32")
        ldgv, npg, Cg = _rows(gv)
        if npg != npix or Cg != Cc:
            raise ValueError("gate_mix_bwd: gv must match feat")
        gfeat = torch.empty(tuple(feat.shape), dtype=torch.float32, device=feat.device)
        ga = torch.empty(tuple(feat.shape[:-1]), dtype=torch.float32, device=feat.device)
    if want_v:
        v = torch.empty(tuple(feat.shape), dtype=torch.float32, device=feat.device)
    check(_lib.lib().kd_gate_mix_bwd(_ptr(feat), dt_of(feat), ldf, _ptr(a), _ptr(gv), ldgv, _ptr(gfeat), Cc, _ptr(ga), _ptr(v), Cc, Cc, npix,
                                     stream_ptr()), "kd_gate_mix_bwd")
    return gfeat, ga, v


def edge_attention_bwd(cs, canny, weights, g_acts):
    """Backward of edge_attention: returns (g_t, g_s, eo_canny) -- gradients w.r.t. the cw and fuse pre-activations (N,H,W) fp32 and the
    cw conv's input [sigmoid(fuse . cs), canny] (N,H,W,2) fp32."""
    _need_cuda(cs, canny, weights, g_acts)
    c8 = cs[..., :8]
    ldc, npix, _ = _rows(c8)
    for t in (canny, g_acts):
        if t.dtype != torch.float32 or t.numel() != npix or not t.is_contiguous():
            raise ValueError("edge_attention_bwd: canny / g_acts must be contiguous fp32 (N,H,W)")
    g_t, g_s = torch.empty_like(g_acts), torch.empty_like(g_acts)
    eo_canny = torch.empty(tuple(g_acts.shape) + (2,), dtype=torch.float32, device=cs.device)
    check(_lib.lib().kd_edge_attention_bwd(dt_of(cs), _ptr(c8), ldc, _ptr(canny), _ptr(weights), _ptr(g_acts), _ptr(g_t), _ptr(g_s), _ptr(eo_canny),
                                           npix, stream_ptr()), "kd_edge_attention_bwd")
    return g_t, g_s, eo_canny


def rank1_add(y, g, w, accumulate=True):
    """y[p][c] (+)= g[p] * w[c]; y (..., C) view, g fp32 one value per pixel, w fp32 (C,)."""
    _need_cuda(y, g, w)
    ldy, npix, Cc = _rows(y)
    w = w.detach().float().contiguous()
    if g.dtype != torch.float32 or g.numel() != npix or not g.is_contiguous() or w.numel() != Cc:
        raise ValueError("rank1_add: g must be contiguous fp32 with one value per pixel, w (C,)")
    check(_lib.lib().kd_rank1_add(dt_of(y), _ptr(y), ldy, _ptr(g), _ptr(w), Cc, npix, int(accumulate), stream_ptr()), "kd_rank1_add")
    return y


# ------------------------------------------------------------------------------------- losses
def view3(t):
    """(N,C,*spatial) logical tensor (any of NCHW / channels_last / (N,C)) -> kd_view3 + (N,C,P)."""
    mat = getattr(t, "materialize", None)     # lazy.LazyLogits: a raw pointer is wanted, so the tensor has to exist
    if mat is not None:
        t = mat()
    if t.dim() == 2:
        N, Cc = t.shape
        return View3(t.data_ptr(), dt_of(t), t.stride(0), t.stride(1), 0), (N, Cc, 1)
    if t.dim() != 4:
        raise ValueError("loss operands must be (N,C) or (N,C,H,W)")
    N, Cc, H, W = t.shape
    sN, sC, sH, sW = t.stride()
    if H > 1 and sH != W * sW:
        raise ValueError(f"loss operand rows are not uniformly strided: stride {t.stride()}")
    return View3(t.data_ptr(), dt_of(t), sN, sC, sW), (N, Cc, H * W)


_ws_cache = {}


def loss_workspace(N, Cc, P, device):
    need = _lib.lib().kd_loss_workspace(N, Cc, P)
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = _ws(need, device, 0)
        _ws_cache[key] = ws
    return ws, need


def _loss_common(s, t):
    _need_cuda(s, t)
    if s.shape != t.shape:
        raise ValueError(f"loss: inputs {tuple(s.shape)} vs targets {tuple(t.shape)}")
    vs, dims = view3(s)
    vt, _ = view3(t)
    return vs, vt, dims


# The profiler's `kernel` field of every loss entry point: the kernel family that runs (csrc/losses.hip picks the member by layout,
# dtype and class count).
_LOSS_KERNELS = {
    "kd_kldiv": "pair_kernel<kld> / pair_nhwc_kernel<kld>",
    "kd_jsdiv": "pair_kernel<jsd> / pair_nhwc_kernel<jsd>",
    "kd_ensemble_kldiv": "pair_kernel<ekl> / pair_nhwc_kernel<ekl>",
    "kd_hint_mse": "mse_vec_kernel / mse_strided_kernel",
    "kd_weighted_hint_mse": "whmse_kernel",
    "kd_topk_hint_mse": "topk_sums_kernel + topk_select_kernel + topk_grad_kernel",
    "kd_ce2d": "ce2d_kernel / ce2d_nhwc_kernel",
    "kd_ce2d_up": "ce2d_up_kernel",
    "kd_kldiv_up": "pair_up_kernel<kld>",
    "kd_jsdiv_up": "pair_up_kernel<jsd>",
    "kd_focal_up": "focal_up_kernel",
    "kd_logit_metrics_up": "logit_metrics_up_kernel",
    "kd_kldiv_multi": "kd_kldiv_multi",
    "kd_softmax_mean": "kd_softmax_mean",
    "kd_focal": "focal_kernel",
    "kd_focal_grad": "focal_grad_kernel",
}


def _pair_loss(fn, label, s, t, extra, want_grad, grad_scale):
    """The two-operand criteria share one call shape: fn(s, t, *extra, N, C, P, loss, grad or NULL, grad_scale, workspace, bytes,
    stream) -> (loss, grad or None).  extra: the criterion's own operands, or a function of (N, C, P) that checks and returns them
    (after the checks of s and t)."""
    vs, vt, (N, Cc, P) = _loss_common(s, t)
    if callable(extra):
        extra = extra(N, Cc, P)
    loss = torch.empty((), dtype=torch.float32, device=s.device)
    grad = torch.empty_like(s) if want_grad else None
    vg = view3(grad)[0] if want_grad else None
    ws, need = loss_workspace(N, Cc, P, s.device)
    e0 = _prof_start()
    own = [_ptr(e) if torch.is_tensor(e) else e for e in extra]      # (`extra` keeps a tensor operand alive over the call)
    check(getattr(_lib.lib(), fn)(C.byref(vs), C.byref(vt), *own, N, Cc, P, _ptr(loss), C.byref(vg) if vg is not None else None,
                                  C.c_float(grad_scale), _ptr(ws), need, stream_ptr()), fn)
    _prof_stop(e0, "loss", _nbytes(s, t, grad), f"{label} {N}x{Cc}x{P}", _LOSS_KERNELS[fn])
    return loss, grad


def kldiv(s, t, temperature=1.0, want_grad=True, grad_scale=1.0):
    return _pair_loss("kd_kldiv", "kldiv", s, t, (C.c_float(temperature),), want_grad, grad_scale)


def hint_mse(s, t, num_classes=19, want_grad=True, grad_scale=1.0):
    return _pair_loss("kd_hint_mse", "hint mse", s, t, (C.c_float(num_classes),), want_grad, grad_scale)


def weighted_hint_mse(s, t, w, want_grad=True, grad_scale=1.0):
    def weights(N, Cc, P):
        _need_cuda(w)
        wf = w.detach().float().contiguous()
        if tuple(wf.shape) not in ((Cc,), (N, Cc)):
            raise ValueError(f"weighted_hint_mse: filter_weight must be (C,) or (N,C), got {tuple(wf.shape)}")
        return wf, int(wf.dim() == 2)
    return _pair_loss("kd_weighted_hint_mse", "weighted hint mse", s, t, weights, want_grad, grad_scale)


def _class_weight(weight, Cc, device):
    w = weight.detach().to(device=device, dtype=torch.float32).contiguous()
    if w.numel() != Cc:
        raise ValueError("class weights: one per class")
    return w


def ce2d(x, target, ignore_index=255, weight=None, size_average=True):
    _need_cuda(x, target)
    vx, (N, Cc, P) = view3(x)
    tgt = target.contiguous()
    if tgt.dtype != torch.int64 or tgt.numel() != N * P:
        raise ValueError("ce2d: target must be int64 (N,H,W)")
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws, need = loss_workspace(N, Cc, P, x.device)
    e0 = _prof_start()
    if weight is not None or not size_average:
        w = _class_weight(weight, Cc, x.device) if weight is not None else None
        check(_lib.lib().kd_ce2d_weighted(C.byref(vx), _ptr(tgt), _ptr(w) if w is not None else None, int(not size_average), ignore_index, N, Cc, P,
                                          _ptr(loss), _ptr(ws), need, stream_ptr()), "kd_ce2d_weighted")
    else:
        check(_lib.lib().kd_ce2d(C.byref(vx), _ptr(tgt), ignore_index, N, Cc, P, _ptr(loss), _ptr(ws), need, stream_ptr()), "kd_ce2d")
    _prof_stop(e0, "loss", _nbytes(x, tgt), f"ce2d {N}x{Cc}x{P}", _LOSS_KERNELS["kd_ce2d"])
    return loss


def _lowres_ok(*lows):
    for t in lows:
        if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("low-resolution logits must be dense fp32 (N,h,w,C)")


def _up_prologue(who, lows, size, target=None):
    """What the *_up wrappers check and allocate alike -> ((N, h, w, C, H, W), target or None, workspace, bytes)."""
    _need_cuda(*lows, target)
    _lowres_ok(*lows)
    if any(t.shape != lows[0].shape for t in lows[1:]):
        raise ValueError(f"{who}: shape mismatch")
    N, h, w, Cc = lows[0].shape
    H, W = size
    tgt = None
    if target is not None:
        tgt = target.contiguous()
        if tgt.dtype != torch.int64 or tgt.numel() != N * H * W:
            raise ValueError(f"{who}: target must be int64 (N,H,W)")
    ws, need = loss_workspace(N, Cc, H * W, lows[0].device)
    return (N, h, w, Cc, H, W), tgt, ws, need


def ce2d_up(x_lo, target, size, ignore_index=255, align_corners=True):
    """ce2d(upsample_bilinear(x_lo, size), target) without the full-resolution tensor (kd_ce2d_up)."""
    (N, h, w, Cc, H, W), tgt, ws, need = _up_prologue("ce2d_up", (x_lo,), size, target)
    loss = torch.empty((), dtype=torch.float32, device=x_lo.device)
    e0 = _prof_start()
    check(_lib.lib().kd_ce2d_up(_ptr(x_lo), _ptr(tgt), ignore_index, N, h, w, Cc, H, W, int(bool(align_corners)), _ptr(loss), _ptr(ws),
                                need, stream_ptr()), "kd_ce2d_up")
    _prof_stop(e0, "loss", _nbytes(x_lo, tgt), f"ce2d from {h}x{w} logits at {H}x{W}", _LOSS_KERNELS["kd_ce2d_up"])
    return loss


def kldiv_up(s_lo, t_lo, size, temperature=1.0, align_corners=True):
    """kldiv(upsample_bilinear(s_lo, size), upsample_bilinear(t_lo, size)) forward, without the full-resolution tensors."""
    (N, h, w, Cc, H, W), _, ws, need = _up_prologue("kldiv_up", (s_lo, t_lo), size)
    loss = torch.empty((), dtype=torch.float32, device=s_lo.device)
    e0 = _prof_start()
    check(_lib.lib().kd_kldiv_up(_ptr(s_lo), _ptr(t_lo), C.c_float(temperature), N, h, w, Cc, H, W, int(bool(align_corners)), _ptr(loss),
                                 _ptr(ws), need, stream_ptr()), "kd_kldiv_up")
    _prof_stop(e0, "loss", _nbytes(s_lo, t_lo), f"kldiv from {h}x{w} logits at {H}x{W}", _LOSS_KERNELS["kd_kldiv_up"])
    return loss


def jsdiv_up(s_lo, t_lo, size, temperature=1.0, align_corners=True):
    """jsdiv(upsample_bilinear(s_lo, size), upsample_bilinear(t_lo, size)) forward, without the full-resolution tensors."""
    (N, h, w, Cc, H, W), _, ws, need = _up_prologue("jsdiv_up", (s_lo, t_lo), size)
    loss = torch.empty((), dtype=torch.float32, device=s_lo.device)
    e0 = _prof_start()
    check(_lib.lib().kd_jsdiv_up(_ptr(s_lo), _ptr(t_lo), C.c_float(temperature), N, h, w, Cc, H, W, int(bool(align_corners)), _ptr(loss),
                                 _ptr(ws), need, stream_ptr()), "kd_jsdiv_up")
    _prof_stop(e0, "loss", _nbytes(s_lo, t_lo), f"jsdiv from {h}x{w} logits at {H}x{W}", _LOSS_KERNELS["kd_jsdiv_up"])
    return loss


class MetricsUnsupported(_lib.KdccError):
    """logit_metrics_up on a class count / resampling ratio kd_logit_metrics_up does not take: compose ce2d_up / hint_mse / confusion."""


def logit_metrics_up(s_lo, t_lo, target, size, ignore_index=255, align_corners=True, conf_s=None, conf_t=None, accumulate=False):
    """The analysis step's logged metrics in one pass over both low-resolution logit tensors (kd_logit_metrics_up).
    Returns (out, conf_s, conf_t): out fp32 (3,) = [ce2d(up(s), target), ce2d(up(t), target), mean (up(s) - up(t))^2]; conf_*
    int64 (C,C) [label][prediction] as confusion() of each up-sampled tensor (added to the given matrices when accumulate).
    Raises MetricsUnsupported (nothing launched) outside the kernel's limits."""
    (N, h, w, Cc, H, W), tgt, ws, need = _up_prologue("logit_metrics_up", (s_lo, t_lo), size, target)
    if conf_s is None or conf_t is None:
        if accumulate:
            raise ValueError("logit_metrics_up: accumulate needs both confusion matrices")
        conf_s = torch.empty((Cc, Cc), dtype=torch.int64, device=s_lo.device)
        conf_t = torch.empty((Cc, Cc), dtype=torch.int64, device=s_lo.device)
    for cf in (conf_s, conf_t):
        _need_cuda(cf)
        if cf.dtype != torch.int64 or tuple(cf.shape) != (Cc, Cc) or not cf.is_contiguous():
            raise ValueError("logit_metrics_up: conf must be a contiguous int64 (C, C) tensor")
    out = torch.empty(3, dtype=torch.float32, device=s_lo.device)
    e0 = _prof_start()
    rc = _lib.lib().kd_logit_metrics_up(_ptr(s_lo), _ptr(t_lo), _ptr(tgt), ignore_index, N, h, w, Cc, H, W, int(bool(align_corners)), _ptr(out),
                                        _ptr(conf_s), _ptr(conf_t), int(bool(accumulate)), _ptr(ws), need, stream_ptr())
    if rc == _lib.KD_ERR_UNSUPPORTED:
        msg = _lib.lib().kd_last_error()
        raise MetricsUnsupported(f"kd_logit_metrics_up: {msg.decode() if msg else ''}")
    check(rc, "kd_logit_metrics_up")
    _prof_stop(e0, "loss", _nbytes(s_lo, t_lo, tgt), f"logit metrics from {h}x{w} logits at {H}x{W}", _LOSS_KERNELS["kd_logit_metrics_up"])
    return out, conf_s, conf_t


def ce2d_grad(x, target, ignore_index=255, grad_scale=1.0, weight=None, size_average=True):
    """d ce2d / d x, same layout as x."""
    _need_cuda(x, target)
    vx, (N, Cc, P) = view3(x)
    tgt = target.contiguous()
    if tgt.dtype != torch.int64 or tgt.numel() != N * P:
        raise ValueError("ce2d_grad: target must be int64 with one label per pixel")
    grad = torch.empty_like(x)
    vg, _ = view3(grad)
    ws, need = loss_workspace(N, Cc, P, x.device)
    if weight is not None or not size_average:
        w = _class_weight(weight, Cc, x.device) if weight is not None else None
        check(_lib.lib().kd_ce2d_weighted_grad(C.byref(vx), _ptr(tgt), _ptr(w) if w is not None else None, int(not size_average), ignore_index, N, Cc, P,
                                               C.byref(vg), C.c_float(grad_scale), _ptr(ws), need, stream_ptr()), "kd_ce2d_weighted_grad")
        return grad
    check(_lib.lib().kd_ce2d_grad(C.byref(vx), _ptr(tgt), ignore_index, N, Cc, P, C.byref(vg), C.c_float(grad_scale), _ptr(ws), need,
                                  stream_ptr()), "kd_ce2d_grad")
    return grad


def confusion(x, target, conf=None, accumulate=False):
    """conf (C,C) int64 [label][prediction] of argmax_c x vs target; pixels whose label is outside [0, C) are skipped."""
    _need_cuda(x, target, conf)
    vx, (N, Cc, P) = view3(x)
    tgt = target.contiguous()
    if tgt.dtype != torch.int64 or tgt.numel() != N * P:
        raise ValueError("confusion: target must be int64 with one label per pixel")
    if conf is None:
        conf, accumulate = torch.empty((Cc, Cc), dtype=torch.int64, device=x.device), False
    if conf.dtype != torch.int64 or tuple(conf.shape) != (Cc, Cc) or not conf.is_contiguous():
        raise ValueError("confusion: conf must be a contiguous int64 (C, C) tensor")
    check(_lib.lib().kd_confusion(C.byref(vx), _ptr(tgt), N, Cc, P, _ptr(conf), int(accumulate), stream_ptr()), "kd_confusion")
    return conf


def jsdiv(s, t, temperature=1.0, want_grad=True, grad_scale=1.0):
    """JSDivergenceLoss (losses/JSDiv.py:19-26) and its gradient w.r.t. s (t constant), one pass (kd_jsdiv)."""
    return _pair_loss("kd_jsdiv", "jsdiv", s, t, (C.c_float(temperature),), want_grad, grad_scale)


def ensemble_kldiv(s, t, want_grad=True, grad_scale=1.0):
    """EnsembleKLDivergenceLoss (losses/EnsembleKLDiv.py:17-21): t are probabilities (kd_ensemble_kldiv)."""
    return _pair_loss("kd_ensemble_kldiv", "ensemble kldiv", s, t, (), want_grad, grad_scale)


def _multi_views(ts, weights, dims, what):
    """kd_multi_targets of `ts` (each of logical shape `dims`) with one weight each.  The count is passed on as it is -- the
    library refuses 0 or more than KD_MULTI_MAX operands with an error code."""
    ts, weights = list(ts), [float(w) for w in weights]
    if len(weights) != len(ts):
        raise ValueError(f"{what}: {len(ts)} operands but {len(weights)} weights")
    mt = MultiTargets()
    mt.n = len(ts)
    for k, t in enumerate(ts[:_lib.KD_MULTI_MAX]):
        v, d = view3(t)
        if d != dims:
            raise ValueError(f"{what}: operand {k} is {d}, expected {dims}")
        mt.t[k] = v
        mt.w[k] = weights[k]
    return mt


def kldiv_multi(s, targets, weights, temperature=1.0, labels=None, ignore_index=255, kd_scale=1.0, sup_scale=1.0, want_grad=True):
    """The ensemble criterion in one pass (kd_kldiv_multi): kd = sum_k w_k KLDivergenceLoss(T)(s, t_k) / sum_k w_k,
    sup = CrossEntropyLoss2d(ignore_index)(s, labels) (0 without labels), total = kd_scale * kd + sup_scale * sup and
    d total / d s.  -> (kd, sup, total, grad): three 0-dim fp32 views of one device buffer, grad like s (None without want_grad)."""
    targets = list(targets)
    _need_cuda(s, labels, *targets)
    vs, dims = view3(s)
    N, Cc, P = dims
    mt = _multi_views(targets, weights, dims, "kldiv_multi")
    tgt = None
    if labels is not None:
        tgt = labels.contiguous()
        if tgt.dtype != torch.int64 or tgt.numel() != N * P:
            raise ValueError("kldiv_multi: labels must be int64 with one label per pixel")
    losses = torch.empty(3, dtype=torch.float32, device=s.device)
    grad = torch.empty_like(s) if want_grad else None
    vg = view3(grad)[0] if want_grad else None
    ws, need = loss_workspace(N, Cc, P, s.device)
    e0 = _prof_start()
    check(_lib.lib().kd_kldiv_multi(C.byref(vs), C.byref(mt), C.c_float(temperature), _ptr(tgt), int(ignore_index), C.c_float(kd_scale),
                                    C.c_float(sup_scale), N, Cc, P, _ptr(losses), C.byref(vg) if vg is not None else None, _ptr(ws), need,
                                    stream_ptr()), "kd_kldiv_multi")
    _prof_stop(e0, "loss", _nbytes(s, grad, tgt, *targets), f"kldiv multi x{len(targets)} {N}x{Cc}x{P}", _LOSS_KERNELS["kd_kldiv_multi"])
    return losses[0], losses[1], losses[2], grad


def softmax_mean(logits, weights, temperature=1.0):
    """sum_k w_k softmax(x_k / T, dim=1) / sum_k w_k as fp32 in the layout of the first operand (kd_softmax_mean): the reference's
    ensemble_predict, and the probabilities EnsembleKLDivergenceLoss takes as its target."""
    logits = list(logits)
    _need_cuda(*logits)
    if not logits:
        mt = MultiTargets()
        check(_lib.lib().kd_softmax_mean(C.byref(mt), C.c_float(temperature), 1, 1, 1, None, stream_ptr()), "kd_softmax_mean")
    dims = view3(logits[0])[1]
    N, Cc, P = dims
    mt = _multi_views(logits, weights, dims, "softmax_mean")
    first = logits[0].materialize() if hasattr(logits[0], "materialize") else logits[0]
    out = torch.empty_like(first, dtype=torch.float32)
    vo, _ = view3(out)
    e0 = _prof_start()
    check(_lib.lib().kd_softmax_mean(C.byref(mt), C.c_float(temperature), N, Cc, P, C.byref(vo), stream_ptr()), "kd_softmax_mean")
    _prof_stop(e0, "loss", _nbytes(out, *logits), f"softmax mean x{len(logits)} {N}x{Cc}x{P}", _LOSS_KERNELS["kd_softmax_mean"])
    return out


_FOCAL_RED = {"none": 0, "mean": 1, "sum": 2}


def _focal_red(reduction, allowed=("none", "mean", "sum")):
    if reduction not in allowed:
        raise ValueError(f"focal: reduction must be one of {allowed}, got {reduction!r}")
    return _FOCAL_RED[reduction]


def _focal_target(x_shape_np, target):
    N, P = x_shape_np
    tgt = target.contiguous()
    if tgt.dtype != torch.int64 or tgt.numel() != N * P:
        raise ValueError("focal: target must be int64 with one label per pixel")
    return tgt


def focal(x, target, gamma, alpha=None, ignore_index=-100, reduction="mean", want_maps=False):
    """FocalLoss (losses/FocalLoss.py:15-28) forward (kd_focal) -> (loss or None for 'none', stats, a_map, ce_map).  stats: fp64 (3,)
    device sums (a, ce, weight) for focal_grad; a_map / ce_map: fp32 (N,P) per-pixel (1-p_y')^gamma and weighted CE, when
    want_maps or reduction == 'none'."""
    _need_cuda(x, target)
    red = _focal_red(reduction)
    vx, (N, Cc, P) = view3(x)
    tgt = _focal_target((N, P), target)
    w = _class_weight(alpha, Cc, x.device) if alpha is not None else None
    loss = torch.empty((), dtype=torch.float32, device=x.device) if red else None
    stats = torch.empty(3, dtype=torch.float64, device=x.device)
    maps = want_maps or red == 0
    amap = torch.empty((N, P), dtype=torch.float32, device=x.device) if maps else None
    cemap = torch.empty((N, P), dtype=torch.float32, device=x.device) if maps else None
    ws, need = loss_workspace(N, Cc, P, x.device)
    e0 = _prof_start()
    check(_lib.lib().kd_focal(C.byref(vx), _ptr(tgt), _ptr(w), C.c_float(gamma), int(ignore_index), red, N, Cc, P, _ptr(loss), _ptr(stats),
                              _ptr(amap), _ptr(cemap), _ptr(ws), need, stream_ptr()), "kd_focal")
    _prof_stop(e0, "loss", _nbytes(x, tgt, amap, cemap), f"focal {N}x{Cc}x{P}", _LOSS_KERNELS["kd_focal"])
    return loss, stats, amap, cemap


def focal_grad(x, target, gamma, alpha, ignore_index, reduction, upstream, stats=None, a_map=None, ce_map=None):
    """d focal / d x times the upstream gradient (kd_focal_grad): a device scalar for 'mean' / 'sum' (with the forward's stats),
    the (N,N,*spatial) gradient of the outer product for 'none' (with the forward's maps).  No host sync."""
    _need_cuda(x, target, upstream)
    red = _focal_red(reduction)
    vx, (N, Cc, P) = view3(x)
    tgt = _focal_target((N, P), target)
    w = _class_weight(alpha, Cc, x.device) if alpha is not None else None
    up = upstream.detach().to(torch.float32).contiguous()
    if (red and up.numel() != 1) or (not red and up.numel() != N * N * P):
        raise ValueError(f"focal_grad: upstream gradient of {up.numel()} elements for reduction {reduction!r}")
    if red and stats is None or not red and (a_map is None or ce_map is None):
        raise ValueError("focal_grad: needs the forward's stats ('mean' / 'sum') or maps ('none')")
    grad = torch.empty_like(x)
    vg, _ = view3(grad)
    e0 = _prof_start()
    check(_lib.lib().kd_focal_grad(C.byref(vx), _ptr(tgt), _ptr(w), C.c_float(gamma), int(ignore_index), red, N, Cc, P, _ptr(stats), _ptr(up),
                                   _ptr(a_map), _ptr(ce_map), C.byref(vg), stream_ptr()), "kd_focal_grad")
    _prof_stop(e0, "loss", _nbytes(x, tgt, grad), f"focal grad {N}x{Cc}x{P}", _LOSS_KERNELS["kd_focal_grad"])
    return grad


def focal_up(x_lo, target, size, gamma, alpha=None, ignore_index=-100, reduction="mean", align_corners=True):
    """focal(upsample_bilinear(x_lo, size), target) 'mean' / 'sum' forward without the full-resolution tensor (kd_focal_up)
    -> (loss, stats)."""
    _need_cuda(x_lo, target)
    _lowres_ok(x_lo)
    red = _focal_red(reduction, ("mean", "sum"))      # (checked between the operands and the labels, whose message is focal's own)
    (N, h, w, Cc, H, W), _, ws, need = _up_prologue("focal_up", (x_lo,), size)
    tgt = _focal_target((N, H * W), target)
    wt = _class_weight(alpha, Cc, x_lo.device) if alpha is not None else None
    loss = torch.empty((), dtype=torch.float32, device=x_lo.device)
    stats = torch.empty(3, dtype=torch.float64, device=x_lo.device)
    e0 = _prof_start()
    check(_lib.lib().kd_focal_up(_ptr(x_lo), _ptr(tgt), _ptr(wt), C.c_float(gamma), int(ignore_index), red, N, h, w, Cc, H, W,
                                 int(bool(align_corners)), _ptr(loss), _ptr(stats), _ptr(ws), need, stream_ptr()), "kd_focal_up")
    _prof_stop(e0, "loss", _nbytes(x_lo, tgt), f"focal from {h}x{w} logits at {H}x{W}", _LOSS_KERNELS["kd_focal_up"])
    return loss, stats


_topk_ws = {}


def topk_hint_mse(s, t, k, want_grad=True, grad_scale=1.0, want_mask=False):
    """TopkHintMSELoss (losses/WeightedHintMSELoss.py:28-44) with k channels kept per sample (kd_topk_hint_mse) ->
    (loss, grad, mask or None)."""
    vs, vt, (N, Cc, P) = _loss_common(s, t)
    if s.dim() != 4:
        raise ValueError(f"topk_hint_mse: 4-D (N,C,H,W) operands only, got {tuple(s.shape)}")
    k = int(k)
    if not 1 <= k <= Cc:
        raise ValueError(f"topk_hint_mse: keeps k = {k} of {Cc} channels; need 1 <= k <= C (topk * C rounded down is 0?)")
    loss = torch.empty((), dtype=torch.float32, device=s.device)
    grad = torch.empty_like(s) if want_grad else None
    vg = view3(grad)[0] if want_grad else None
    mask = torch.empty((N, Cc), dtype=torch.float32, device=s.device) if want_mask else None
    need = _lib.lib().kd_topk_hint_workspace(N, Cc, P)
    key = (s.device, torch.cuda.current_stream().cuda_stream)
    ws = _topk_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _topk_ws[key] = _ws(need, s.device, 0)
    e0 = _prof_start()
    check(_lib.lib().kd_topk_hint_mse(C.byref(vs), C.byref(vt), k, N, Cc, P, _ptr(loss), C.byref(vg) if vg is not None else None,
                                      C.c_float(grad_scale), _ptr(mask), _ptr(ws), need, stream_ptr()), "kd_topk_hint_mse")
    _prof_stop(e0, "loss", _nbytes(s, t, grad), f"top-{k} hint mse {N}x{Cc}x{P}", _LOSS_KERNELS["kd_topk_hint_mse"])
    return loss, grad, mask


def radam_step_multi(items):
    """items: [(p, g, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay), ...] -- kd_radam_step for all of them in one
    launch per 48 tensors; same arithmetic per element as radam_step."""
    if not items:
        return
    arr = (_lib.RadamTensor * len(items))()
    for i, (p, g, m, v, step, lr, beta1, beta2, eps, wd) in enumerate(items):
        _need_cuda(p, g, m, v)
        for t in (p, g, m, v):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise ValueError("radam_step_multi: fp32 contiguous tensors of equal size required")
        a = arr[i]
        a.p, a.g, a.exp_avg, a.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        a.n, a.step = p.numel(), int(step)
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = lr, beta1, beta2, eps, wd
    check(_lib.lib().kd_radam_step_multi(arr, len(items), stream_ptr()), "kd_radam_step_multi")
    # the kernel wrote through raw pointers: tell autograd / version-keyed caches (engine weight packs) about it
    for (p, _, m, v, *_rest) in items:
        for t in (p, m, v):
            torch.autograd.graph.increment_version(t)


def radam_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    _need_cuda(p, g, m, v)
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
            raise ValueError("radam_step: fp32 contiguous tensors of equal size required")
    check(_lib.lib().kd_radam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), int(step), C.c_float(lr), C.c_float(beta1),
                                   C.c_float(beta2), C.c_float(eps), C.c_float(weight_decay), stream_ptr()), "kd_radam_step")
    # the kernel wrote through raw pointers: tell autograd / version-keyed caches (engine weight packs) about it
    for t in (p, m, v):
        torch.autograd.graph.increment_version(t)


OPT_RULES = {"sgd": _lib.KD_OPT_SGD, "adam": _lib.KD_OPT_ADAM, "adamw_ref": _lib.KD_OPT_ADAMW_REF}
OPT_FIRST, OPT_NESTEROV, OPT_AMSGRAD, OPT_MAXIMIZE = _lib.KD_OPT_FIRST, _lib.KD_OPT_NESTEROV, _lib.KD_OPT_AMSGRAD, _lib.KD_OPT_MAXIMIZE


def optim_launch_shape(rule):
    """(tensors one launch of `rule` holds, elements one block steps) of kd_optim_step_multi."""
    mt, be = C.c_int32(), C.c_int32()
    check(_lib.lib().kd_optim_launch_shape(OPT_RULES[rule] if isinstance(rule, str) else int(rule), C.byref(mt), C.byref(be)),
          "kd_optim_launch_shape")
    return mt.value, be.value


def optim_step_multi(rule, items):
    """One optimizer step for many tensors (kd_optim_step_multi, csrc/optim.hip): rule "sgd" (torch.optim.SGD), "adam"
    (torch.optim.Adam) or "adamw_ref" (the reference's AdamW, utils/optim/radam.py:179-250), the arithmetic stated in include/kdcc.h.
    items: [(p, g, states, step, flags, hp), ...]
      states  the state tensors the rule updates in place: sgd (momentum_buffer,) or (); adam (exp_avg, exp_avg_sq[,
              max_exp_avg_sq]); adamw_ref (exp_avg, exp_avg_sq)
      step    the tensor's step count after the increment (sgd: unused)
      flags   OPT_FIRST (sgd: the momentum buffer is new, it is written and not read) | OPT_NESTEROV | OPT_AMSGRAD | OPT_MAXIMIZE
      hp      (lr, weight_decay, eps, momentum, dampening, beta1, beta2, warmup): Python floats, they reach the library as doubles
    Runs on the current stream; allocates, copies and synchronises nothing."""
    if not items:
        return
    rule = OPT_RULES[rule] if isinstance(rule, str) else int(rule)
    arr = (_lib.OptimTensor * len(items))()
    f32 = torch.float32
    for i, (p, g, states, step, flags, hp) in enumerate(items):
        n = p.numel()
        for t in (p, g, *states):
            if not t.is_cuda:
                raise _lib.KdccError("kdcc kernels need device tensors (there is no CPU fallback)")
            if t.dtype != f32 or not t.is_contiguous() or t.numel() != n:
                raise TypeError("optim_step_multi: fp32 contiguous tensors of equal size required")
        sp = [s.data_ptr() for s in states]
        arr[i] = _lib.OptimTensor(p.data_ptr(), g.data_ptr(), (_lib.c_vp * 3)(*sp), n, int(step), int(flags), 0, *hp)
    check(_lib.lib().kd_optim_step_multi(rule, arr, len(items), stream_ptr()), "kd_optim_step_multi")
    # the kernel wrote through raw pointers: tell autograd / version-keyed caches (engine weight packs) about it
    torch.autograd.graph.increment_version([t for (p, _, states, *_rest) in items for t in (p, *states)])


# ------------------------------------------------------------------------- HRNetV2 + OCR (csrc/hrnet_ops.hip)
def _f32_views(name, *ts):
    for t in ts:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise (_lib.KdccError if not t.is_cuda else TypeError)(f"{name}: fp32 device tensors only (there is no CPU fallback)")


def _pixel_ld(t):
    """nhwc_ld() that also takes extents of 1, whose strides torch leaves arbitrary (a 1x1 source of the fuse sum)."""
    if t.dim() != 4 or (t.shape[3] > 1 and t.stride(3) != 1):
        raise ValueError(f"expected an (N,H,W,C) tensor with dense channels, got shape {tuple(t.shape)} stride {t.stride()}")
    N, H, W, Cc = t.shape
    ld = t.stride(2) if W > 1 else t.stride(1) if H > 1 else t.stride(0) if N > 1 else Cc
    if ld < Cc or (H > 1 and t.stride(1) != W * ld) or (N > 1 and t.stride(0) != H * W * ld):
        raise ValueError(f"not a pixel-strided NHWC view: shape {tuple(t.shape)} stride {t.stride()}")
    return ld


def _hr_views(ts, shape_nc, name):
    arr = (_lib.HrView * len(ts))()
    for i, t in enumerate(ts):
        if t is None:
            arr[i].ptr, arr[i].H, arr[i].W, arr[i].ld = None, 0, 0, 0
            continue
        if t.dim() != 4 or (t.shape[0], t.shape[3]) != shape_nc:
            raise ValueError(f"{name}: source {i} has shape {tuple(t.shape)}, expected (N,H,W,C) with (N, C) = {shape_nc}")
        arr[i].ptr, arr[i].H, arr[i].W, arr[i].ld = t.data_ptr(), t.shape[1], t.shape[2], _pixel_ld(t)
    return arr


def hr_fuse(srcs, size=None, out=None):
    """y = relu(sum_s sample(srcs[s])): 1..4 (N,H_s,W_s,C) fp32 views; a source of the output size (Ho, Wo) -- srcs[0]'s unless
    `size` / `out` says otherwise -- is read directly, a coarser one sampled bilinearly (align_corners=True)."""
    _f32_views("hr_fuse", *srcs, out)
    N, Cc = srcs[0].shape[0], srcs[0].shape[3]
    Ho, Wo = (out.shape[1], out.shape[2]) if out is not None else (size or srcs[0].shape[1:3])
    if out is None:
        out = torch.empty((N, Ho, Wo, Cc), dtype=torch.float32, device=srcs[0].device)
    if tuple(out.shape) != (N, Ho, Wo, Cc):
        raise ValueError("hr_fuse: bad output view")
    arr = _hr_views(srcs, (N, Cc), "hr_fuse")
    check(_lib.lib().kd_hr_fuse_fwd(arr, len(srcs), _ptr(out), _pixel_ld(out), N, Ho, Wo, Cc, stream_ptr()), "kd_hr_fuse_fwd")
    return out


def hr_fuse_bwd(gy, y, sizes, need=None):
    """Gradients of hr_fuse's sources from gy and the forward's y: sizes = [(H_s, W_s)], need[s] False skips that source (None)."""
    _f32_views("hr_fuse_bwd", gy, y)
    N, Ho, Wo, Cc = y.shape
    if tuple(gy.shape) != (N, Ho, Wo, Cc):
        raise ValueError("hr_fuse_bwd: gy must have y's shape")
    need = [True] * len(sizes) if need is None else list(need)
    outs = [torch.empty((N, h, w, Cc), dtype=torch.float32, device=y.device) if nd else None for (h, w), nd in zip(sizes, need)]
    arr = _hr_views(outs, (N, Cc), "hr_fuse_bwd")
    check(_lib.lib().kd_hr_fuse_bwd(_ptr(gy), _pixel_ld(gy), _ptr(y), _pixel_ld(y), arr, len(outs), N, Ho, Wo, Cc, stream_ptr()), "kd_hr_fuse_bwd")
    return outs


def _rows3(t, name):
    """(N, HW, C) view with dense channels and one pixel stride -> that stride."""
    if t.dim() != 3 or t.stride(2) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)) or t.stride(1) < t.shape[2]:
        raise ValueError(f"{name}: expected an (N,HW,C) view with dense channels, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.stride(1)


def ocr_gather(logits, feats):
    """logits (N,HW,K), feats (N,HW,C) -> ctx (N,K,C) = softmax_HW(logits)^T . feats, and (mx, lse) (N,K) for the backward."""
    _f32_views("ocr_gather", logits, feats)
    N, HW, K = logits.shape
    Cc = feats.shape[2]
    if tuple(feats.shape[:2]) != (N, HW):
        raise ValueError("ocr_gather: logits and feats must share (N, HW)")
    ctx = torch.empty((N, K, Cc), dtype=torch.float32, device=feats.device)
    mx, lse = torch.empty((N, K), dtype=torch.float32, device=feats.device), torch.empty((N, K), dtype=torch.float32, device=feats.device)
    need = _lib.lib().kd_ocr_gather_workspace(N, HW, K, Cc)
    ws = _ws(need, feats.device)
    check(_lib.lib().kd_ocr_gather_fwd(_ptr(logits), _rows3(logits, "ocr_gather"), _ptr(feats), _rows3(feats, "ocr_gather"), _ptr(ctx), _ptr(mx),
                                       _ptr(lse), N, HW, K, Cc, _ptr(ws), need, stream_ptr()), "kd_ocr_gather_fwd")
    return ctx, mx, lse


def ocr_gather_bwd(gctx, ctx, logits, feats, lse):
    """-> (d_feats (N,HW,C), d_logits (N,HW,K)); the probabilities are recomputed from logits and lse."""
    _f32_views("ocr_gather_bwd", gctx, ctx, logits, feats, lse)
    N, HW, K = logits.shape
    Cc = feats.shape[2]
    gctx, ctx, lse = gctx.contiguous(), ctx.contiguous(), lse.contiguous()
    if tuple(gctx.shape) != (N, K, Cc) or tuple(ctx.shape) != (N, K, Cc) or tuple(lse.shape) != (N, K):
        raise ValueError("ocr_gather_bwd: operand mismatch")
    d_feats = torch.empty((N, HW, Cc), dtype=torch.float32, device=feats.device)
    d_logits = torch.empty((N, HW, K), dtype=torch.float32, device=feats.device)
    need = _lib.lib().kd_ocr_gather_workspace(N, HW, K, Cc)
    ws = _ws(need, feats.device)
    check(_lib.lib().kd_ocr_gather_bwd(_ptr(gctx), _ptr(ctx), _ptr(logits), _rows3(logits, "ocr_gather_bwd"), _ptr(feats),
                                       _rows3(feats, "ocr_gather_bwd"), _ptr(lse), _ptr(d_feats), Cc, _ptr(d_logits), K, N, HW, K, Cc, _ptr(ws),
                                       need, stream_ptr()), "kd_ocr_gather_bwd")
    return d_feats, d_logits


def ocr_attend(query, key, value, scale=None):
    """query (N,HW,Ck), key / value (N,K,Ck) -> ctx (N,HW,Ck) = softmax_K(scale * query . key^T) . value; scale defaults to Ck^-0.5."""
    _f32_views("ocr_attend", query, key, value)
    N, HW, Ck = query.shape
    K = key.shape[1]
    key, value = key.contiguous(), value.contiguous()
    if tuple(key.shape) != (N, K, Ck) or tuple(value.shape) != (N, K, Ck):
        raise ValueError("ocr_attend: key / value must be (N,K,Ck)")
    scale = float(Ck) ** -0.5 if scale is None else float(scale)
    ctx = torch.empty((N, HW, Ck), dtype=torch.float32, device=query.device)
    check(_lib.lib().kd_ocr_attend_fwd(_ptr(query), _rows3(query, "ocr_attend"), _ptr(key), _ptr(value), _ptr(ctx), Ck, N, HW, K, Ck,
                                       C.c_float(scale), stream_ptr()), "kd_ocr_attend_fwd")
    return ctx


def ocr_attend_bwd(g, query, key, value, scale=None):
    """-> (d_query, d_key, d_value) of ocr_attend from g = d ctx (N,HW,Ck)."""
    _f32_views("ocr_attend_bwd", g, query, key, value)
    N, HW, Ck = query.shape
    K = key.shape[1]
    key, value = key.contiguous(), value.contiguous()
    if tuple(g.shape) != (N, HW, Ck) or tuple(key.shape) != (N, K, Ck) or tuple(value.shape) != (N, K, Ck):
        raise ValueError("ocr_attend_bwd: operand mismatch")
    scale = float(Ck) ** -0.5 if scale is None else float(scale)
    dq = torch.empty((N, HW, Ck), dtype=torch.float32, device=query.device)
    dk, dv = torch.empty_like(key), torch.empty_like(value)
    need = _lib.lib().kd_ocr_attend_workspace(N, HW, K, Ck)
    ws = _ws(need, query.device)
    check(_lib.lib().kd_ocr_attend_bwd(_ptr(g), _rows3(g, "ocr_attend_bwd"), _ptr(query), _rows3(query, "ocr_attend_bwd"), _ptr(key), _ptr(value),
                                       _ptr(dq), Ck, _ptr(dk), _ptr(dv), N, HW, K, Ck, C.c_float(scale), _ptr(ws), need, stream_ptr()),
          "kd_ocr_attend_bwd")
    return dq, dk, dv


# ------------------------------------------------------------------------- CIFAR batches (data_loader)
def check_cifar_params(params, n):
    """ValueError unless `params` is an int32 (B,4) table of rows [index, dy, dx, flip] with index in [0, n), dy, dx in [0, 8] and
    flip in {0, 1}.  Reads the values: a device table is copied to the host first (a synchronisation)."""
    if params.dim() != 2 or params.shape[1] != 4 or params.shape[0] < 1 or params.dtype != torch.int32:
        raise ValueError(f"cifar_batch: params must be an int32 (B,4) table, got {params.dtype} {tuple(params.shape)}")
    p = params.detach().cpu()
    lo, hi = p.amin(0).tolist(), p.amax(0).tolist()
    for col, (name, top) in enumerate((("index", n - 1), ("dy", 8), ("dx", 8), ("flip", 1))):
        if lo[col] < 0 or hi[col] > top:
            raise ValueError(f"cifar_batch: {name} spans [{lo[col]}, {hi[col]}], allowed [0, {top}]")


def cifar_batch(data, labels, params, table, out, labels_out=None, validated=False):
    """One batch of the CIFAR loaders in one launch (kd_cifar_batch): crop, flip, ToTensor and Normalize as a gather.
    data (n,32,32,3) uint8 and labels (n,) int64: the resident dataset; params int32 (B,4) rows [index, dy, dx, flip]; table (3,256)
    of out's dtype (fp32 / bf16).  out is (B,3,32,32)-logical: a dense NCHW tensor, or NHWC storage with any pixel stride ld >= 3
    (channels_last, or the channel prefix of a wider (B,32,32,ld) buffer) -- then the kernel writes the WHOLE stride of every pixel,
    zeros in channels [3, ld), so the buffer may come from torch.empty.  -> (out, labels_out).
    params is checked on the host (check_cifar_params; for a device table that is a copy and a synchronisation) unless the caller
    has done so already and says validated=True, as the loaders do once per epoch."""
    _need_cuda(data, labels, params, table, out, labels_out)
    n = data.shape[0]
    if data.dtype != torch.uint8 or data.dim() != 4 or tuple(data.shape[1:]) != (32, 32, 3) or n < 1 or not data.is_contiguous():
        raise ValueError(f"cifar_batch: data must be a contiguous uint8 (n,32,32,3) tensor, got {data.dtype} {tuple(data.shape)}")
    if labels.dtype != torch.int64 or tuple(labels.shape) != (n,) or not labels.is_contiguous():
        raise ValueError(f"cifar_batch: labels must be a contiguous int64 ({n},) tensor")
    if not validated:
        check_cifar_params(params, n)
    B = params.shape[0]
    if params.dtype != torch.int32 or tuple(params.shape) != (B, 4) or not params.is_contiguous():
        raise ValueError("cifar_batch: params must be a contiguous int32 (B,4) table")
    dt = dt_of(out)
    if table.dtype != out.dtype or tuple(table.shape) != (3, 256) or not table.is_contiguous():
        raise ValueError(f"cifar_batch: table must be a contiguous (3,256) tensor of out's dtype {out.dtype}")
    if tuple(out.shape) != (B, 3, 32, 32):
        raise ValueError(f"cifar_batch: out must be ({B},3,32,32)-logical, got {tuple(out.shape)}")
    if out.is_contiguous():
        layout, ld = _lib.KD_CIFAR_NCHW, 3
    else:
        layout, ld = _lib.KD_CIFAR_NHWC, nhwc_ld(out.permute(0, 2, 3, 1))
    if labels_out is None:
        labels_out = torch.empty((B,), dtype=torch.int64, device=out.device)
    elif labels_out.dtype != torch.int64 or tuple(labels_out.shape) != (B,) or not labels_out.is_contiguous():
        raise ValueError(f"cifar_batch: labels_out must be a contiguous int64 ({B},) tensor")
    check(_lib.lib().kd_cifar_batch(_ptr(data), _ptr(labels), n, _ptr(params), B, _ptr(table), dt, layout, _ptr(out), ld, _ptr(labels_out),
                                    stream_ptr()), "kd_cifar_batch")
    return out, labels_out


# ------------------------------------------------------------------------- Cityscapes batches (data_loader)
SEG_HDR, SEG_ENTRY, SEG_TAPS, SEG_TX, SEG_TY, SEG_CAP_C, SEG_CAP_R, SEG_MAX_RADIUS = 32, 11, 9, 32, 16, 74, 42, 5


def _seg_bad(what):
    raise ValueError(f"check_seg_params: {what}")


def _seg_check_axis(ent, near, extent, tile, cap, name):
    """One axis of an expanded table: entries (B,S,11) and nearest indices (B,S)."""
    xmin, taps = ent[..., 0], ent[..., 1]
    pad = xmin < 0
    if bool((pad & ((xmin != -1) | (taps != 0))).any()):
        _seg_bad(f"a {name} entry is neither a window nor the pad marker [-1, 0]")
    if bool((~pad & ((taps < 1) | (taps > SEG_TAPS) | (xmin + taps > extent))).any()):
        _seg_bad(f"a {name} tap window leaves the source [0, {extent}) or has more than {SEG_TAPS} taps")
    if bool(((near < -1) | (near >= extent) | ((near < 0) != pad)).any()):
        _seg_bad(f"a nearest {name} index is outside [-1, {extent}) or disagrees with the pad")
    B, S = xmin.shape
    fill = (-S) % tile          # whole tiles: the tail counts as pad
    lo = torch.nn.functional.pad(torch.where(pad, torch.full_like(xmin, 1 << 30), xmin), (0, fill), value=1 << 30).view(B, -1, tile).amin(2)
    hi = torch.nn.functional.pad(torch.where(pad, torch.zeros_like(xmin), xmin + taps), (0, fill), value=0).view(B, -1, tile).amax(2)
    if bool((hi - lo > cap).any()):
        _seg_bad(f"the {name} windows of one tile span more than {cap} source pixels (a scale below 0.5)")


def check_seg_params(params, n, H, W, S=None):
    """ValueError unless `params` is an int32 table of Cityscapes rows (data_loader/seg_tables.py) the kernels may be launched on:
    header rows (B,32), or with S the expanded rows (B, 32 + 24 S) of kd_seg_crop.  Index in [0, n), w, h >= 1, flip and the jitter
    flag 0 / 1, the order a permutation, the hue byte in [0, 255], the radius in [0, 5]; with S also the crop window inside the
    padded scaled image, every tap window inside the source, at most 9 taps, every tile's windows within what the kernel stages,
    nearest indices inside the source.  Reads the values: a device table is copied to the host first (a synchronisation)."""
    width = SEG_HDR if S is None else SEG_HDR + (2 * SEG_ENTRY + 2) * S
    if params.dim() != 2 or params.shape[0] < 1 or params.shape[1] != width or params.dtype != torch.int32:
        _seg_bad(f"params must be an int32 (B,{width}) table, got {params.dtype} {tuple(params.shape)}")
    p = params.detach().cpu()
    idx, w, h, pw, ph, x1, y1, flip = (p[:, i] for i in range(8))
    if bool(((idx < 0) | (idx >= n)).any()):
        _seg_bad(f"index spans [{int(idx.min())}, {int(idx.max())}], allowed [0, {n - 1}]")
    if bool(((w < 1) | (h < 1)).any()):
        _seg_bad("a scaled size w, h below 1")
    if bool(((flip < 0) | (flip > 1) | (p[:, 17] < 0) | (p[:, 17] > 1)).any()):
        _seg_bad("flip and the jitter flag are 0 or 1")
    if not bool((p[:, 8:12].sort(1).values == torch.arange(4)).all()):
        _seg_bad("the order of the colour operations is not a permutation of 0..3")
    if bool(((p[:, 15] < 0) | (p[:, 15] > 255)).any()):
        _seg_bad("the hue shift is a byte")
    if bool(((p[:, 16] < 0) | (p[:, 16] > SEG_MAX_RADIUS)).any()):
        _seg_bad(f"blur radius spans [{int(p[:, 16].min())}, {int(p[:, 16].max())}], allowed [0, {SEG_MAX_RADIUS}]")
    if S is None:
        return
    if bool(((pw < 0) | (ph < 0) | (x1 < 0) | (y1 < 0) | (x1 + S > w + 2 * pw) | (y1 + S > h + 2 * ph)).any()):
        _seg_bad(f"the {S} x {S} crop window leaves the padded scaled image")
    B = p.shape[0]
    ent = p[:, SEG_HDR:SEG_HDR + 2 * SEG_ENTRY * S].view(B, 2, S, SEG_ENTRY)
    near = p[:, SEG_HDR + 2 * SEG_ENTRY * S:].view(B, 2, S)
    _seg_check_axis(ent[:, 0], near[:, 0], W, SEG_TX, SEG_CAP_C, "column")
    _seg_check_axis(ent[:, 1], near[:, 1], H, SEG_TY, SEG_CAP_R, "row")


def _seg_bytes(t, shape, name):
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous uint8 {tuple(shape)} tensor, got {t.dtype} {tuple(t.shape)}")


def _seg_table(params, width, name):
    if params.dtype != torch.int32 or params.dim() != 2 or params.shape[1] < width or params.stride(1) != 1 or params.shape[0] < 1:
        raise ValueError(f"{name}: params must be an int32 (B, >= {width}) table with dense rows")
    return params.shape[0], params.stride(0) if params.shape[0] > 1 else params.shape[1]


def seg_crop(data, targets, params, S, img_out=None, mask_out=None, validated=False):
    """Resample + pad + crop + flip (kd_seg_crop): data (n,H,W,3) and targets (n,H,W) uint8, the resident dataset; params the
    expanded int32 table (B, 32 + 24 S).  -> (img (B,S,S,3), mask (B,S,S)) uint8, PIL's bicubic / nearest resize, the reference's pad,
    crop and flip, bit for bit.  params is checked on the host (check_seg_params) unless validated=True."""
    _need_cuda(data, targets, params, img_out, mask_out)
    if data.dim() != 4 or data.shape[3] != 3:
        raise ValueError(f"seg_crop: data must be (n,H,W,3), got {tuple(data.shape)}")
    n, H, W = data.shape[:3]
    _seg_bytes(data, (n, H, W, 3), "seg_crop: data")
    _seg_bytes(targets, (n, H, W), "seg_crop: targets")
    if not validated:
        check_seg_params(params, n, H, W, S)
    B, pld = _seg_table(params, SEG_HDR + (2 * SEG_ENTRY + 2) * S, "seg_crop")
    img_out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=data.device) if img_out is None else img_out
    mask_out = torch.empty((B, S, S), dtype=torch.uint8, device=data.device) if mask_out is None else mask_out
    _seg_bytes(img_out, (B, S, S, 3), "seg_crop: img_out")
    _seg_bytes(mask_out, (B, S, S), "seg_crop: mask_out")
    check(_lib.lib().kd_seg_crop(_ptr(data), _ptr(targets), n, H, W, _ptr(params), pld, B, S, _ptr(img_out), _ptr(mask_out), stream_ptr()),
          "kd_seg_crop")
    return img_out, mask_out


def seg_jitter(img, params, workspace=None, validated=False):
    """The colour jitter (kd_seg_jitter) in place on img (B,S,S,3) uint8, for every row of params (B, >= 32) whose jitter flag is set:
    PIL's brightness, contrast, saturation and hue in the row's order, bit for bit.  -> img."""
    _need_cuda(img, params, workspace)
    if img.dim() != 4 or img.shape[1] != img.shape[2] or img.shape[3] != 3:
        raise ValueError(f"seg_jitter: img must be (B,S,S,3), got {tuple(img.shape)}")
    B, S = img.shape[:2]
    _seg_bytes(img, (B, S, S, 3), "seg_jitter: img")
    if _seg_table(params, SEG_HDR, "seg_jitter")[0] != B:
        raise ValueError(f"seg_jitter: {params.shape[0]} rows for {B} images")
    if not validated:
        check_seg_params(params[:, :SEG_HDR], 2 ** 31 - 1, 1, 1)
    need = _lib.lib().kd_seg_jitter_workspace(B)
    if workspace is None:
        workspace = _ws(need, img.device, 0)
    check(_lib.lib().kd_seg_jitter(_ptr(img), _ptr(params), _seg_table(params, SEG_HDR, "seg_jitter")[1], B, S, _ptr(workspace),
                                   workspace.numel() * workspace.element_size(), stream_ptr()), "kd_seg_jitter")
    return img


def seg_finish(img, mask, params, table, out, mask_out=None, use_index=False, blur=False, validated=False):
    """Blur + quantise + normalise + layout (kd_seg_finish).  img (n,H,W,3) and mask (n,H,W) uint8: a batch of crops (image b of the
    batch is sample b) or, with use_index, the resident dataset (sample b is image params[b, 0]).  blur: the Gaussian of every row
    whose radius is not 0, scipy's in double, truncated to bytes.  table (3,256) of out's dtype; out (B,3,H,W)-logical, dense NCHW or
    NHWC storage with any pixel stride ld >= 3, whose whole stride the kernel writes (zeros behind channel 3).
    -> (out, mask_out int64 (B,H,W))."""
    _need_cuda(img, mask, params, table, out, mask_out)
    if img.dim() != 4 or img.shape[3] != 3:
        raise ValueError(f"seg_finish: img must be (n,H,W,3), got {tuple(img.shape)}")
    n, H, W = img.shape[:3]
    _seg_bytes(img, (n, H, W, 3), "seg_finish: img")
    _seg_bytes(mask, (n, H, W), "seg_finish: mask")
    B, pld = _seg_table(params, SEG_HDR, "seg_finish")
    if not validated:
        check_seg_params(params[:, :SEG_HDR], n if use_index else 2 ** 31 - 1, H, W)
    if not use_index and n < B:
        raise ValueError(f"seg_finish: {n} images for {B} rows")
    dt = dt_of(out)
    if table.dtype != out.dtype or tuple(table.shape) != (3, 256) or not table.is_contiguous():
        raise ValueError(f"seg_finish: table must be a contiguous (3,256) tensor of out's dtype {out.dtype}")
    if tuple(out.shape) != (B, 3, H, W):
        raise ValueError(f"seg_finish: out must be ({B},3,{H},{W})-logical, got {tuple(out.shape)}")
    if out.is_contiguous():
        layout, ld = _lib.KD_SEG_NCHW, 3
    else:
        layout, ld = _lib.KD_SEG_NHWC, nhwc_ld(out.permute(0, 2, 3, 1))
    if mask_out is None:
        mask_out = torch.empty((B, H, W), dtype=torch.int64, device=out.device)
    elif mask_out.dtype != torch.int64 or tuple(mask_out.shape) != (B, H, W) or not mask_out.is_contiguous():
        raise ValueError(f"seg_finish: mask_out must be a contiguous int64 ({B},{H},{W}) tensor")
    check(_lib.lib().kd_seg_finish(_ptr(img), _ptr(mask), n, H, W, _ptr(params), pld, B, int(bool(use_index)), int(bool(blur)), _ptr(table), dt,
                                   layout, _ptr(out), ld, _ptr(mask_out), stream_ptr()), "kd_seg_finish")
    return out, mask_out


# ------------------------------------------------------------------------- per-tile class statistics (data_loader.uniform)
SEG_STATS_MAX_CLASSES, SEG_MAX_SIDE = 64, 1 << 15
_SEG_STATS_HOST_BYTES = 1 << 26         # label bytes the host path compares at once


def _host_class_stats(targets, tile, num_classes, out):
    """The sums of kd_seg_class_stats with torch integer ops on host tensors: what the kernel is a restatement of."""
    n, th, tw = out.shape[:3]
    ar = torch.arange(tile, dtype=torch.int64)
    step = max(1, _SEG_STATS_HOST_BYTES // (th * tw * tile * tile))
    for s in range(0, n, step):
        t = targets[s:s + step, :th * tile, :tw * tile].reshape(-1, th, tile, tw, tile)         # (b, ty, y, tx, x)
        for c in range(num_classes):
            m = t == c
            col = m.sum(2, dtype=torch.int64)               # (b, ty, tx, x): the class's pixels per tile column
            row = m.sum(4, dtype=torch.int64)               # (b, ty, y, tx): per tile row
            out[s:s + step, :, :, c, 0] = col.sum(3)
            out[s:s + step, :, :, c, 1] = (col * ar).sum(3)
            out[s:s + step, :, :, c, 2] = (row * ar[:, None]).sum(2)
    return out


def seg_class_stats(targets, tile, num_classes=19):
    """int64 (n, H // tile, W // tile, num_classes, 3) = [count, sum of x, sum of y] of the pixels of every class inside every
    tile x tile tile of the uint8 label maps targets (n,H,W), x and y relative to the tile's origin (kd_seg_class_stats; see
    include/kdcc.h).  Remainder rows and columns belong to no tile; a tile larger than the image gives an empty tensor and no launch;
    255 and every value >= num_classes count nowhere.  Device tensors run the kernel; host tensors the same exact integer sums with
    torch ops, equal bit for bit."""
    if targets.dtype != torch.uint8 or targets.dim() != 3 or targets.shape[0] < 1 or not targets.is_contiguous():
        raise ValueError(f"seg_class_stats: targets must be a contiguous uint8 (n,H,W) tensor, got {targets.dtype} {tuple(targets.shape)}")
    n, H, W = targets.shape
    tile, num_classes = int(tile), int(num_classes)
    if tile < 1:
        raise ValueError(f"seg_class_stats: a tile of {tile} pixels")
    if not 1 <= num_classes <= SEG_STATS_MAX_CLASSES:
        raise ValueError(f"seg_class_stats: num_classes {num_classes} outside [1, {SEG_STATS_MAX_CLASSES}]")
    if not (1 <= H <= SEG_MAX_SIDE and 1 <= W <= SEG_MAX_SIDE):
        raise ValueError(f"seg_class_stats: H = {H}, W = {W} outside [1, {SEG_MAX_SIDE}]")
    th, tw = (H // tile, W // tile) if tile <= min(H, W) else (0, 0)
    out = torch.empty((n, th, tw, num_classes, 3), dtype=torch.int64, device=targets.device)
    if th == 0:
        return out
    if not targets.is_cuda:
        return _host_class_stats(targets, tile, num_classes, out)
    check(_lib.lib().kd_seg_class_stats(_ptr(targets), n, H, W, tile, num_classes, _ptr(out), stream_ptr()), "kd_seg_class_stats")
    return out
