"""Both sides of every gate of the conv forward and weight-gradient dispatchers (tests/_conv_dispatch_cases.py), one process,
default environment: each row asserts the kernel the dispatcher chose (kd_debug_last_kernel and the counted log) against the row
and against the pure-Python restatement evaluated for this device's CU count, and compares the result with the CPU oracle's
double-accumulating loops (oracle/oracle.c) on the same storage-rounded inputs at the bars of tests/test_ops_gpu.py.

Outputs are channel slices of wider buffers prefilled with a sentinel that must survive outside the slice; epilogue rows check
out_raw and out_act separately; rows that compute one layer on two kernels are also compared with each other.  The weight-gradient
rows run with a workspace of exactly the bytes the ABI's *_workspace() returns (ops allocates that many), so a bound that is too
small is a KD_ERR_WORKSPACE failure here."""
import collections
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _conv_dispatch_cases as T  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from test_ops_gpu import DT, assert_close, host_nchw, selected  # noqa: E402

SENTINEL = 7.0
FWD = T.cases_of("conv2d", "conv2d_dgrad")
WG = T.cases_of("conv2d_wgrad", "pw_wgrad")


@pytest.fixture(scope="module")
def K():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    assert torch.cuda.is_available()
    return ops


def q(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[dt]).float().numpy()


def randn(key, shape, dt, scale=1.0, offset=0.0):
    rng = np.random.default_rng(T.seed_of(*key))
    return q(rng.standard_normal(shape, dtype=np.float32) * np.float32(scale) + np.float32(offset), dt)


def pad_rows(a, rows):
    return a if not rows else np.concatenate([a, np.zeros(a.shape[:2] + (rows,) + a.shape[3:], a.dtype)], axis=2)


def view(a_nchw, dt, ld=None, off=None, fill=0.0, torch_dtype=None):
    """NHWC device copy of an NCHW array as a channel slice [off, off + C) of a buffer with `ld` channels per pixel."""
    t = torch.from_numpy(np.ascontiguousarray(a_nchw.transpose(0, 2, 3, 1))).to(torch_dtype or DT[dt]).cuda()
    if ld is None:
        return t, None
    N, H, W, C = t.shape
    if off is None:
        off = 8 if ld >= C + 8 else 0
    buf = torch.full((N, H, W, ld), fill, dtype=t.dtype, device="cuda")
    buf[..., off:off + C] = t
    return buf[..., off:off + C], buf


def out_view(shape, Cout, torch_dtype, ld, off):
    N, Ho, Wo = shape
    buf = torch.full((N, Ho, Wo, ld), SENTINEL, dtype=torch_dtype, device="cuda")
    return buf[..., off:off + Cout], buf


def sentinel_survives(buf, off, C, what):
    assert bool((buf[..., :off] == SENTINEL).all()) and bool((buf[..., off + C:] == SENTINEL).all()), f"{what}: written outside its channel slice"


_ORACLE = collections.OrderedDict()


def cached(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
        while len(_ORACLE) > 3:
            _ORACLE.popitem(last=False)
    _ORACLE.move_to_end(key)
    return _ORACLE[key]


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def check_selection(c, log):
    from kdcc_amd import _lib
    selected(c["kernel"], c["id"])
    want = T.predict(c, device_cus())
    assert want["kernel"] == _lib.last_kernel(), f"{c['id']}: the restated dispatcher predicts {want['kernel']} on {device_cus()} CUs"
    assert log.counts.get(c["kernel"], 0) == 1, f"{c['id']}: kernel log {log.counts}"
    for n in T.EPILOGUE_NOTES:
        assert log.counts.get(n, 0) == (1 if n in want["notes"] else 0), f"{c['id']}: epilogue note {n}: log {log.counts}, predicted {want['notes']}"
    return want


RESULTS = {}


def run_forward(K, c):
    from kdcc_amd import _lib
    dt = c["dt"]
    N, H, W, Cin, Cout, k, s, p, d = c["shape"]
    zr = c.get("zero_rows", 0)
    Hd = H - zr
    sums = c.get("sums")
    if c["entry"] == "conv2d_dgrad":
        # the forward layer Cin -> Cout; the launch is its input gradient: dy (Cout channels) -> dx (Cin channels)
        Cs, Co = Cout, Cin
        xin = randn(("dy", dt, N, H, W, Cout, d), (N, Cout, H, W), dt)
        w = randn(("w", dt, Cin, Cout, k), (Cout, Cin, k, k), dt, scale=(2.0 / (Cout * k * k)) ** 0.5)
        conv = cached((c["id"], "conv"), lambda: orc.conv2d_dgrad(xin, w, (N, Cin, H, W), stride=1, pad=p, dil=d).astype(np.float64))
        wp = K.pack_conv_weight(torch.from_numpy(w).cuda(), DT[dt], mode=_lib.KD_PACK_DGRAD)
        Ho, Wo = H, W
    else:
        Cs, Co = Cin + c.get("cin2", 0), Cout
        xoff, woff = (1.0, 0.5) if sums == "bn" else (0.0, 0.0)          # well-conditioned channel sums: outputs with a common sign
        wscale = (2.0 / (Cs * k * k)) ** 0.5
        xin = pad_rows(randn(("x", dt, N, Hd, W, Cs, xoff), (N, Cs, Hd, W), dt, offset=xoff), zr)
        wc = c.get("wkey_cout", Cout)
        w = randn(("w", dt, Cs, wc if wc >= Cout else Cout, k, woff), (max(wc, Cout), Cs, k, k), dt, scale=wscale, offset=woff * wscale)[:Cout]
        conv = cached((dt, N, Hd, zr, W, Cs, Cout, wc, k, s, p, d, xoff),
                      lambda: orc.conv2d_fwd(xin, w, stride=s, pad=p, dil=d).astype(np.float64))
        wp = K.pack_conv_weight(torch.from_numpy(np.ascontiguousarray(w)).cuda(), DT[dt])
        Ho, Wo = conv.shape[2:]
    zo = zr if Ho == H else 0
    opn = lambda name, relu=False: pad_rows((lambda a: q(np.maximum(a, 0), dt) if relu else a)(
        randn((name, dt, N, Ho - zo, Wo, max(Co, c.get("wkey_cout", 0))), (N, max(Co, c.get("wkey_cout", 0)), Ho - zo, Wo), dt)), zo)[:, :Co]
    vec = lambda name, sc, off: (np.random.default_rng(T.seed_of(name, Co)).standard_normal(Co) * sc + off).astype(np.float32)
    bc = lambda v: v[None, :, None, None]
    ops_ = c["ops"]
    pre, mask, post = (opn("pre") if "pre" in ops_ else None, opn("mask", relu=True) if "mask" in ops_ else None,
                       opn("post") if "post" in ops_ else None)
    mscale, ascale, ashift = vec("mscale", 0.2, 1.0), vec("ascale", 0.2, 1.0), vec("ashift", 0.3, 0.0)
    ref = conv
    if pre is not None:
        ref = ref + pre
    if mask is not None:
        ref = np.where(mask > 0, ref * bc(mscale), 0.0)
    g = ref
    if post is not None:
        ref = ref + post
    want_act = "act" in c["outs"] or c.get("cls")
    act_ref = np.maximum(ref * bc(ascale) + bc(ashift), 0) if want_act else None

    cu = lambda v: torch.from_numpy(v).cuda()
    mis = c.get("misalign")
    x_d, _ = view(xin[:, :Cin] if c.get("cin2") else xin, dt, ld=(Cin if c.get("cin2") else Cs) + 16)
    x2_d = view(xin[:, Cin:], dt, ld=c["cin2"] + 8)[0] if c.get("cin2") else None
    opv = lambda a, name, pad: None if a is None else view(a, dt, ld=Co + pad, off=4 if mis == name else 8)[0]
    raw_dtype = torch.float32 if c.get("raw_f32") else DT[dt]
    raw_off, act_off = (4 if mis == "raw" else 16), Co
    out_raw, raw_buf = out_view((N, Ho, Wo), Co, raw_dtype, Co + 32, raw_off) if "raw" in c["outs"] else (None, None)
    out_act, act_buf = out_view((N, Ho, Wo), Co, DT[dt], 2 * Co, act_off) if "act" in c["outs"] else (None, None)
    kw = dict(res_pre=opv(pre, "pre", 16), mask=opv(mask, "mask", 16), mask_scale=cu(mscale) if mask is not None else None,
              res_post=opv(post, "post", 24), out_raw=out_raw, out_act=out_act)
    if want_act:
        kw.update(act_scale=cu(ascale), act_shift=cu(ashift), act_relu=True)
    bn_sums, out_sums = ([] if sums == "bn" else None), ([] if sums == "out" else None)
    cls_out = cls_buf = None
    if c.get("cls"):
        ncls = c["cls"]
        wcls = randn(("wcls", dt, ncls, Co), (ncls, Co, 1, 1), dt, scale=0.08)
        wcd = torch.zeros((32, Co, 1, 1), device="cuda")
        wcd[:ncls] = cu(wcls)
        assert K.conv_cls_ok(x_d, Co, k, d), f"{c['id']}: kd_conv2d_cls_supported refuses the shape the restatement sends to conv_row_lw_kernel"
        cls_out, cls_buf = out_view((N, Ho, Wo), ncls, torch.float32, 32, 0)
        kw.update(cls_w=K.pack_conv_weight(wcd, DT[dt]), cls_out=cls_out)
    with _lib.kernel_log() as log:
        if c["entry"] == "conv2d_dgrad":
            K.conv2d(x_d, wp, 1, d * (k - 1) - p, d, bn_sums=bn_sums, **kw)
        else:
            K.conv2d(x_d, wp, s, p, d, x2=x2_d, bn_sums=bn_sums, out_sums=out_sums, **kw)
        torch.cuda.synchronize()
    want = check_selection(c, log)

    got = {}
    if out_raw is not None:
        sentinel_survives(raw_buf, raw_off, Co, f"{c['id']} out_raw")
        got["raw"] = host_nchw(out_raw)
        assert_close(got["raw"], ref, dt, f"{c['id']} raw")
    if out_act is not None:
        sentinel_survives(act_buf, act_off, Co, f"{c['id']} out_act")
        got["act"] = host_nchw(out_act)
        assert_close(got["act"], act_ref, dt, f"{c['id']} act")
    if cls_out is not None:
        sentinel_survives(cls_buf, 0, c["cls"], f"{c['id']} cls_out")
        cls_ref = np.einsum("nchw,kc->nkhw", q(act_ref, dt).astype(np.float64), wcls[:, :, 0, 0].astype(np.float64))
        assert_close(host_nchw(cls_out), cls_ref, dt, f"{c['id']} cls")
    if sums == "bn":
        assert len(bn_sums) == (1 if want["sums_granted"] else 0), f"{c['id']}: kd_conv2d_bn_sums_rows and the restatement disagree"
        if bn_sums:
            # (the bar of test_conv_epilogue_bn_sums: fused sums against fp64 sums of the same expression)
            for name, a, r in (("s1", bn_sums[0][0], g.sum((0, 2, 3))), ("s2", bn_sums[0][1], (g * mask).sum((0, 2, 3)))):
                err = np.abs(a.double().cpu().numpy() - r).max() / (np.abs(r).max() + 1e-6)
                print(f"{c['id']} {name}: {err:.3e} of max")
                assert err < 4e-3, f"{c['id']}: fused {name} off by {err:.3e} of its largest channel"
    if sums == "out":
        assert len(out_sums) == (1 if want["sums_granted"] else 0), f"{c['id']}: kd_conv2d_bn_sums_rows and the restatement disagree"
        if out_sums:
            M = N * Ho * Wo
            part = out_sums[0].cpu().numpy()
            assert part.shape == (M // 128, 2, Co)
            blocks = out_raw.float().reshape(M // 128, 128, Co).sum(1).cpu().numpy()
            np.testing.assert_allclose(part[:, 0], blocks, rtol=2e-5, atol=2e-4)       # (test_conv_output_sums_feed_the_image_pooling's bar)
            assert not part[:, 1].any()
    return got


@pytest.mark.parametrize("c", FWD, ids=T.ids(FWD))
def test_forward_gate(K, c):
    got = run_forward(K, c)
    if "pair" in c or any(o.get("pair", ("",))[0] == c["id"] for o in FWD):
        RESULTS[c["id"]] = got


PAIRS = [c for c in FWD if "pair" in c]


@pytest.mark.parametrize("c", PAIRS, ids=T.ids(PAIRS))
def test_two_kernels_agree_on_one_layer(K, c):
    """Both sides of a gate on the same data: a border error the oracle usage shared with both would not hide here."""
    by_id = {o["id"]: o for o in FWD}
    other, how = c["pair"]
    a = RESULTS[c["id"]] if c["id"] in RESULTS else run_forward(K, c)
    b = RESULTS[other] if other in RESULTS else run_forward(K, by_id[other])
    assert set(a) & set(b)
    for name in sorted(set(a) & set(b)):
        if how == "rows":
            rows = by_id[other]["shape"][1]
            assert_close(a[name][:, :, :rows], b[name], c["dt"], f"{c['id']} vs {other}: {name}")
        else:
            ch = by_id[other]["shape"][4]
            assert_close(a[name][:, :ch], b[name], c["dt"], f"{c['id']} vs {other}: {name}")


@pytest.mark.parametrize("c", WG, ids=T.ids(WG))
def test_weight_gradient_gate(K, c):
    from kdcc_amd import _lib
    dt = c["dt"]
    N, H, W, Cin, Cout, k, s, p, d = c["shape"]
    Ho, Wo = orc.conv_out(H, k, s, p, d), orc.conv_out(W, k, s, p, d)
    x = randn(("wx", dt, N, H, W, Cin), (N, Cin, H, W), dt)
    gy = randn(("wdy", dt, N, Ho, Wo, Cout), (N, Cout, Ho, Wo), dt)
    ref = orc.conv2d_wgrad(x, gy, (Cout, Cin, k, k), stride=s, pad=p, dil=d).astype(np.float64)
    xd, _ = view(x, dt, ld=Cin + c.get("ldx_pad", 16))
    gyd, _ = view(gy, dt, ld=Cout + c["ldy_pad"]) if "ldy_pad" in c else view(gy, dt)
    del x, gy
    want = T.predict(c)
    M = N * Ho * Wo
    if c["entry"] == "pw_wgrad":
        bound = int(_lib.lib().kd_pw_wgrad_workspace(M, Cin, Cout))
    else:
        desc = _lib.ConvDesc(_lib.KD_BF16 if dt == "bf16" else _lib.KD_F32, N, H, W, Cin, Ho, Wo, Cout, k, k, s, p, d, Cin + c.get("ldx_pad", 16))
        bound = int(_lib.lib().kd_conv2d_wgrad_workspace(ctypes.byref(desc)))
    assert bound == want["workspace"], f"{c['id']}: the ABI's workspace bound is {bound}, its restatement gives {want['workspace']}"
    ws = torch.empty(bound, dtype=torch.uint8, device="cuda")          # exactly the bytes the ABI asks for: KD_ERR_WORKSPACE raises below
    dw = torch.full((Cout, Cin, k, k), SENTINEL, device="cuda")
    for acc in (False, True):
        with _lib.kernel_log() as log:
            if c["entry"] == "pw_wgrad":
                K.pw_wgrad(xd, gyd, dw, accumulate=acc, workspace=ws)
            else:
                K.conv2d_wgrad(xd, gyd, dw, s, p, d, accumulate=acc, workspace=ws)
            torch.cuda.synchronize()
        check_selection(c, log)
        assert_close(dw.cpu().numpy(), (2 if acc else 1) * ref, dt, f"{c['id']}{' accumulate' if acc else ''}")


@pytest.mark.parametrize("Cin", T.REFUSED_CIN)
def test_bf16_reduction_depths_under_one_k_stage_pair_are_refused(K, Cin):
    """Why `Cin % 64` of the conv_row_tall_kernel gate has no row: the dispatcher is never asked."""
    from kdcc_amd import _lib
    x = torch.zeros((1, 8, 512, Cin), dtype=torch.bfloat16, device="cuda")
    wp = torch.zeros((128, 3, 3, Cin), dtype=torch.bfloat16, device="cuda")
    out = torch.full((1, 8, 512, 128), SENTINEL, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.KdccError):
        K.conv2d(x, wp, 1, 1, 1, out_raw=out)
    assert bool((out == SENTINEL).all())
