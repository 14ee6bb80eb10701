"""Every dispatch branch of the trunk / backward / small-shape plumbing kernels (csrc/trunk_ops.hip, bwd_ops.hip,
small_ops.hip) against stock torch on the CPU in float64, evaluated on the inputs as stored (tests/_plumbing_cases.py).

Each case asserts the kernel it reached (kd_debug_last_plumbing_kernel), the way selected() does for the convs.
Bars: kernels that move or select values are bitwise; elementwise / interpolation kernels use test_ops_gpu.assert_close (the
project's operator bars); reductions use the recursive-summation bound gamma(L + k) * sum |x_i| with L computed from the shape
(the helpers in _plumbing_cases.py restate the kernel lines they come from).
"""
import numpy as np
import pytest
import torch

import _plumbing_cases as P
from test_ops_gpu import assert_close

pytestmark = pytest.mark.gpu

DT = P.DT


@pytest.fixture(scope="module")
def K():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    assert torch.cuda.is_available()
    return ops


def reached(c):
    from kdcc_amd import _lib
    got = _lib.last_plumbing_kernel()
    assert got == c["kernel"], f"{c['id']}: dispatched to {got}, this case is meant to cover {c['kernel']}"


def dev(a, dt, sliced=False, ld=None, off=8):
    """Device tensor of the storage dtype; sliced: a channel slice (at element `off`) of a wider buffer filled with a sentinel."""
    t = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DT[dt]).cuda()
    if not sliced:
        return t
    C = t.shape[-1]
    ld = ld or C + 16
    buf = torch.full(t.shape[:-1] + (ld,), 7.0, dtype=t.dtype, device="cuda")
    buf[..., off:off + C] = t
    return buf[..., off:off + C]


def out_view(shape, dt, sliced, ld=None, off=8):
    """(view to write, whole buffer): the buffer outside the view must keep its sentinel."""
    if not sliced:
        t = torch.full(shape, 7.0, dtype=DT[dt], device="cuda")
        return t, t
    C = shape[-1]
    ld = ld or C + 16
    buf = torch.full(tuple(shape[:-1]) + (ld,), 7.0, dtype=DT[dt], device="cuda")
    return buf[..., off:off + C], buf


def untouched(view, buf, off=8):
    if view is buf:
        return
    C = view.shape[-1]
    assert bool((buf[..., :off] == 7.0).all()) and bool((buf[..., off + C:] == 7.0).all()), "wrote outside the channel slice"


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def within(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = np.argmax(err - bound)
    print(f"{what}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert (err <= bound).all(), (f"{what}: |err| {err.flat[worst]:.6e} > bound {np.asarray(bound).flat[worst]:.6e} at {worst} "
                                  f"(got {np.asarray(got).flat[worst]!r}, ref {ref.flat[worst]!r})")


# --------------------------------------------------------------------------------------------------------------- reductions
CS = P.cases_of("channel_sums")


@pytest.mark.parametrize("c", CS, ids=P.ids(CS))
def test_channel_sums(K, c):
    from kdcc_amd import _lib
    inp, ref = P.build(c)
    dt = c["dt"]
    kw = dict(ld=c.get("slice_ld"), off=c.get("slice_off", 8))
    g = dev(inp["g"], dt, "g" in c["sliced"], **kw)
    sub = dev(inp["sub"], dt, "sub" in c["sliced"]) if c["sub"] else None
    a = dev(inp["a"], dt, "a" in c["sliced"]) if c["a"] else None
    s1, s2 = K.channel_sums(g, sub=sub, a=a, per_image=c["per_image"])
    reached(c)
    if "ws_bytes" in c:      # the chunk count, through the workspace the dispatcher sizes by it
        N, H, W, C = c["shape"]
        assert _lib.lib().kd_channel_sums_workspace(1, N * H * W, C) == c["ws_bytes"]
    assert tuple(s1.shape) == P.channel_sums_shape(c)
    within(host(s1), ref["s1"], P.channel_sums_bound(c, ref, "s1"), f"{c['id']} s1")
    if c["a"]:
        within(host(s2), ref["s2"], P.channel_sums_bound(c, ref, "s2"), f"{c['id']} s2")
    else:
        assert s2 is None


BS = P.cases_of("bn_sums_finish")


@pytest.mark.parametrize("c", BS, ids=P.ids(BS))
def test_bn_sums_finish(K, c):
    inp, ref = P.build(c)
    s1, s2 = K.bn_sums_finish(torch.from_numpy(inp["part"]).cuda())
    reached(c)
    within(host(s1), ref["s1"], P.bn_sums_finish_bound(c, ref, "s1"), f"{c['id']} s1")
    within(host(s2), ref["s2"], P.bn_sums_finish_bound(c, ref, "s2"), f"{c['id']} s2")


IP = P.cases_of("aspp_image_pool")


@pytest.mark.parametrize("c", IP, ids=P.ids(IP))
def test_aspp_image_pool(K, c):
    inp, ref = P.build(c)
    dt = c["dt"]
    cu = lambda v: torch.from_numpy(v).cuda()
    out, buf = out_view(ref["y"].shape, dt, c["sliced"])
    K.aspp_image_pool(dev(inp["x"], dt), cu(inp["w"]), cu(inp["scale"]), cu(inp["shift"]), out)
    reached(c)
    untouched(out, buf)
    got = host(out)
    assert (got == got[:, :1, :1, :]).all(), "the broadcast is not constant over the pixels"     # a move: exact
    within(got[:, 0, 0, :], ref["v"], ref["bound"], c["id"])


SW = P.cases_of("stem_wgrad")


@pytest.mark.parametrize("c", SW, ids=P.ids(SW))
def test_stem_wgrad(K, c):
    inp, ref = P.build(c)
    ld, off = {"dense": (None, 0), "ld72": (72, 8), "ld68": (68, 4), "off1": (72, 1)}[c["view"]]
    dy = dev(inp["dy"], c["dt"], ld is not None, ld=ld, off=off)
    x = torch.from_numpy(inp["x"]).cuda()
    dw = torch.full((64, 3, 3, 3), 7.0, device="cuda")
    K.stem_wgrad(x, dy, dw)
    reached(c)
    within(host(dw), ref["dw"], P.stem_wgrad_bound(c, ref), c["id"])
    once = dw.clone()
    K.stem_wgrad(x, dy, dw, accumulate=True)
    assert torch.equal(dw, 2 * once), "accumulate=True must add the same gradient again"


DW = P.cases_of("direct_wgrad")


@pytest.mark.parametrize("c", DW, ids=P.ids(DW))
def test_direct_wgrad(K, c):
    inp, ref = P.build(c)
    N, C, H, W, Kk, k, s, p, g, has_b = c["desc"]
    x, dy = torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["dy"]).cuda()
    wshape = (Kk, C // g, k, k)
    dw, db = K.conv2d_direct_wgrad(x, dy, wshape, s, p, 1, g, want_bias=has_b)
    reached(c)
    bw, bb = P.direct_wgrad_bounds(c, ref)
    within(host(dw), ref["dw"], bw, f"{c['id']} dw")
    if has_b:
        within(host(db), ref["db"], bb, f"{c['id']} db")
    else:
        assert db is None
    dw2, db2 = dw.clone(), (db.clone() if has_b else None)
    K.conv2d_direct_wgrad(x, dy, wshape, s, p, 1, g, want_bias=has_b, dw=dw2, db=db2, accumulate=True)
    assert torch.equal(dw2, 2 * dw) and (not has_b or torch.equal(db2, 2 * db)), "accumulate=True must add the same gradient again"


BF = P.cases_of("bn2d_fwd")


@pytest.mark.parametrize("c", BF, ids=P.ids(BF))
def test_bn2d_fwd(K, c):
    inp, ref = P.build(c)
    cu = lambda v: torch.from_numpy(v.copy()).cuda()
    N, C, H, W = c["shape"]
    M = N * H * W
    rm, rv = cu(inp["run_mean"]), cu(inp["run_var"])
    y, mean, invstd = K.bn2d_fwd(cu(inp["x"]), cu(inp["gamma"]), cu(inp["beta"]), rm, rv, c["train"], P.BN_MOM, P.BN_EPS, relu=c["relu"])
    reached(c)
    assert_close(host(y), ref["y"], "f32", f"{c['id']} y")
    if c["train"]:
        # mean: gamma(L + 2) mean |x| (the chain, the division, the store).  invstd = (var + eps)^-1/2 with var a sum of squares
        # about the computed mean: relative error gamma(L + 4) of the sum, plus (mean error)^2 / var from the centre, halved by
        # the square root, plus rsqrt and the store.
        L = P.bn_chain(M)
        bm = P.gamma(L + 2) * ref["absmean"]
        within(host(mean), ref["mean"], bm, f"{c['id']} mean")
        rel = 0.5 * (P.gamma(L + 4) + bm ** 2 / (ref["var"] + P.BN_EPS)) + 4 * P.U
        within(host(invstd), ref["invstd"], rel * ref["invstd"], f"{c['id']} invstd")
        # running statistics: momentum blends of the above (unbiased variance)
        within(host(rm), ref["run_mean"], P.BN_MOM * bm + 3 * P.U * np.abs(ref["run_mean"]) + 2 * P.U * np.abs(inp["run_mean"]), f"{c['id']} running mean")
        within(host(rv), ref["run_var"], (2 * rel + 4 * P.U) * np.abs(ref["run_var"]), f"{c['id']} running var")
    else:
        assert torch.equal(mean.cpu(), torch.from_numpy(inp["run_mean"]))          # eval: the running statistics, untouched
        within(host(invstd), ref["invstd"], 4 * P.U * ref["invstd"], f"{c['id']} invstd")
        assert torch.equal(rm.cpu(), torch.from_numpy(inp["run_mean"])) and torch.equal(rv.cpu(), torch.from_numpy(inp["run_var"]))


BB = P.cases_of("bn2d_bwd")


@pytest.mark.parametrize("c", BB, ids=P.ids(BB))
def test_bn2d_bwd(K, c):
    inp, ref = P.build(c)
    cu = lambda v: torch.from_numpy(v).cuda()
    args = [cu(inp[k]) for k in ("dy", "x", "y", "gamma", "mean", "invstd")]
    dx, dg, db = K.bn2d_bwd(*args, c["train"], relu=c["relu"], need_dx=c["need_dx"])
    reached(c)
    bg, bb = P.bn2d_bwd_bounds(c, ref)
    within(host(dg), ref["dgamma"], bg, f"{c['id']} dgamma")
    within(host(db), ref["dbeta"], bb, f"{c['id']} dbeta")
    if c["need_dx"]:
        assert_close(host(dx), ref["dx"], "f32", f"{c['id']} dx")
    else:
        assert dx is None
    dg2, db2 = dg.clone(), db.clone()
    K.bn2d_bwd(*args, c["train"], relu=c["relu"], need_dx=False, dgamma=dg2, dbeta=db2, accumulate=True)
    assert torch.equal(dg2, 2 * dg) and torch.equal(db2, 2 * db), "accumulate=True must add the same gradients again"


# --------------------------------------------------------------------------------------------------- elementwise, grid-stride
RB = P.cases_of("relu_bn_bwd")


@pytest.mark.parametrize("c", RB, ids=P.ids(RB))
def test_relu_bn_bwd(K, c):
    inp, ref = P.build(c)
    dt = c["dt"]
    out, buf = out_view(c["shape"], dt, "out" in c["sliced"])
    K.relu_bn_bwd(dev(inp["g"], dt, "g" in c["sliced"]), dev(inp["mask"], dt, "mask" in c["sliced"]), torch.from_numpy(inp["scale"]).cuda(),
                  res=dev(inp["res"], dt) if c["res"] else None, out=out)
    reached(c)
    untouched(out, buf)
    assert_close(host(out), ref["y"], dt, c["id"])


BA = P.cases_of("broadcast_add")


@pytest.mark.parametrize("c", BA, ids=P.ids(BA))
def test_broadcast_add(K, c):
    inp, ref = P.build(c)
    dt = c["dt"]
    y = dev(inp["y0"], dt, c["sliced"])
    K.broadcast_add(torch.from_numpy(inp["v"]).cuda(), y, alpha=inp["alpha"], accumulate=bool(c["accumulate"]))
    reached(c)
    if c["accumulate"]:
        assert_close(host(y), ref["y"], dt, c["id"])
    else:       # alpha * v with alpha = 0.5 is exact: the kernel only moves (and, for bf16, rounds) values
        assert torch.equal(y.cpu(), torch.from_numpy(ref["y"]).float().to(DT[dt])), f"{c['id']}: not the exact product"


CC = P.cases_of("copy_cast")


@pytest.mark.parametrize("c", CC, ids=P.ids(CC))
def test_copy_cast(K, c):
    inp, ref = P.build(c)
    N, C, H, W = c["shape"]

    def layout(kind, dtype, fill=None):
        if kind == "nchw":
            t = torch.full((N, C, H, W), 7.0, dtype=dtype, device="cuda")
        elif kind == "cl":
            t = torch.full((N, H, W, C), 7.0, dtype=dtype, device="cuda").permute(0, 3, 1, 2)
        else:
            t = torch.full((N, H, W, C + 13), 7.0, dtype=dtype, device="cuda")[..., 5:5 + C].permute(0, 3, 1, 2)
        if fill is not None:
            t.copy_(fill)
        return t
    src = layout(c["src"], DT[c["sd"]], inp["src"].cuda())
    dst = layout(c["dst"], DT[c["dd"]])
    K.copy_cast(src, dst)
    reached(c)
    assert torch.equal(dst.cpu(), ref["dst"]), f"{c['id']}: not tensor.to(dtype) bit for bit"


ZI = P.cases_of("zero_insert")


@pytest.mark.parametrize("c", ZI, ids=P.ids(ZI))
def test_zero_insert(K, c):
    inp, ref = P.build(c)
    y = K.zero_insert(dev(inp["x"], c["dt"], True), c["stride"], inp["size"])
    reached(c)
    assert torch.equal(y.cpu(), torch.from_numpy(ref["y"]).to(DT[c["dt"]]))


FO = P.cases_of("bn_fold")


@pytest.mark.parametrize("c", FO, ids=P.ids(FO))
def test_bn_fold(K, c):
    inp, ref = P.build(c)
    bn = torch.nn.BatchNorm2d(c["C"], eps=inp["eps"]).cuda().eval()
    with torch.no_grad():
        for t, k in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "mean"), (bn.running_var, "var")):
            t.copy_(torch.from_numpy(inp[k]))
    scale, shift = K.bn_fold(bn)
    reached(c)
    # one division, one square root, one product, one subtraction: a few fp32 roundings of the operands
    within(host(scale), ref["scale"], 4 * P.U * np.abs(ref["scale"]), f"{c['id']} scale")
    within(host(shift), ref["shift"], 4 * P.U * (np.abs(inp["beta"]) + np.abs(inp["mean"] * ref["scale"])), f"{c['id']} shift")
    assert float(scale[3]) == 0.0 and float(shift[3]) == float(inp["beta"][3]), "gamma = 0 must give scale 0 and shift beta"


PG = P.cases_of("bn_eval_param_grads")


@pytest.mark.parametrize("c", PG, ids=P.ids(PG))
def test_bn_eval_param_grads(K, c):
    inp, ref = P.build(c)
    cu = lambda v: torch.from_numpy(v).cuda()
    ops = [cu(inp[k]) for k in ("s1", "s2", "scale", "gamma", "beta")]
    dg, db = torch.full((c["C"],), 7.0, device="cuda"), torch.full((c["C"],), 7.0, device="cuda")
    K.bn_eval_param_grads(*ops, dg, db)
    reached(c)
    # dbeta: one division.  dgamma: product, subtraction (cancellation: bounded by the operands), product, division.
    s1, s2, sc, gm, bt = (inp[k].astype(np.float64) for k in ("s1", "s2", "scale", "gamma", "beta"))
    with np.errstate(divide="ignore", invalid="ignore"):
        bg = np.where((sc != 0) & (gm != 0), 6 * P.U * (np.abs(s2) + np.abs(bt * s1)) / np.abs(sc * gm), 0.0)
    within(host(db), ref["dbeta"], 2 * P.U * np.abs(ref["dbeta"]), f"{c['id']} dbeta")
    within(host(dg), ref["dgamma"], bg, f"{c['id']} dgamma")
    assert float(dg[3]) == 0.0 and float(db[3]) == 0.0, "gamma = 0 must give zero gradients"
    if c["accumulate"]:
        once_g, once_b = dg.clone(), db.clone()
        K.bn_eval_param_grads(*ops, dg, db, accumulate=True)
        assert torch.equal(dg, 2 * once_g) and torch.equal(db, 2 * once_b)


# ------------------------------------------------------------------------------------------------------------------- pooling
MP = P.cases_of("maxpool")


@pytest.mark.parametrize("c", MP, ids=P.ids(MP))
def test_maxpool(K, c):
    inp, ref = P.build(c)
    dt = c["dt"]
    cu = lambda v: torch.from_numpy(v).cuda()
    want_raw, want_act = c["outs"] in ("both", "raw"), c["outs"] in ("both", "act")
    oshape = ref["raw"].shape
    raw, rbuf = out_view(oshape, dt, c["sliced"]) if want_raw else (None, None)
    act, abuf = out_view(oshape, dt, c["sliced"]) if want_act else (None, None)
    r2, a2 = K.maxpool3x3s2(dev(inp["x"], dt, c["sliced"]), cu(inp["scale"]) if want_act else None, cu(inp["shift"]) if want_act else None,
                            want_raw=want_raw, out_raw=raw, out_act=act)
    reached(c)
    if want_raw:
        untouched(raw, rbuf)
        assert torch.equal(r2.cpu(), torch.from_numpy(ref["raw"]).to(DT[dt])), f"{c['id']}: the pooled maximum is a selection: exact"
    else:
        assert r2 is None
    if want_act:
        untouched(act, abuf)
        assert float(np.abs(ref["act"]).max()) > 0
        assert_close(host(a2), ref["act"], dt, f"{c['id']} act")
    else:
        assert a2 is None


def _pool_bwd(K, c, inp, path):
    dt = c["dt"]
    if path == "scalar":     # a pixel stride that is no multiple of 16 bytes: the vector paths refuse, C stays 8
        x, gy = dev(inp["x"], dt, True, ld=c["shape"][3] + 1, off=0), dev(inp["gy"], dt)
    else:
        x, gy = dev(inp["x"], dt), dev(inp["gy"], dt)
    return K.maxpool3x3s2_bwd(x, gy, workspace=path in ("argmax", "dense"))


PB = P.cases_of("maxpool_bwd")


@pytest.mark.parametrize("c", PB, ids=P.ids(PB))
def test_maxpool_bwd(K, c):
    inp, ref = P.build(c)
    got = _pool_bwd(K, c, inp, c["path"])
    reached(c)
    assert_close(host(got), ref["gx"], c["dt"], c["id"])


PB3 = [c for c in PB if c["path"] == "argmax" and c["shape"][3] == 8]


@pytest.mark.parametrize("c", PB3, ids=P.ids(PB3))
def test_maxpool_bwd_three_paths_bit_identical(K, c):
    from kdcc_amd import _lib
    inp, _ = P.build(c)
    outs = {}
    for path, lit in P.POOL_BWD_PATHS.items():
        outs[path] = _pool_bwd(K, c, inp, path)
        assert _lib.last_plumbing_kernel() == lit % c["dt"]
    assert torch.equal(outs["argmax"], outs["gather8"]) and torch.equal(outs["argmax"], outs["scalar"])


# ---------------------------------------------------------------------------------------------------------------- resampling
UP = P.cases_of("upsample")


@pytest.mark.parametrize("c", UP, ids=P.ids(UP))
def test_upsample(K, c):
    inp, ref = P.build(c)
    ld, off = (c["C"] + 16, 8) if c["C"] % 8 == 0 else (c["C"] + 13, 5)
    out, buf = out_view(ref["y"].shape, c["to"], c["sliced"], ld=ld, off=off)
    K.upsample_bilinear_ac(dev(inp["x"], c["ti"], c["C"] % 8 == 0 and c["sliced"]), c["hout"], out=out, align_corners=c["align"])
    reached(c)
    untouched(out, buf, off=off)
    assert_close(host(out), ref["y"], c["to"], c["id"])


UB = P.cases_of("upsample_bwd")


@pytest.mark.parametrize("c", UB, ids=P.ids(UB))
def test_upsample_bwd(K, c):
    inp, ref = P.build(c)
    ld, off = (c["C"] + 16, 8) if c["C"] % 8 == 0 else (c["C"] + 13, 5)
    out, buf = out_view(ref["gx"].shape, c["tx"], c["sliced"], ld=ld, off=off)
    K.upsample_bilinear_ac_bwd(dev(inp["gy"], c["tg"]), c["hin"], out=out, align_corners=c["align"])
    reached(c)
    untouched(out, buf, off=off)
    assert_close(host(out), ref["gx"], c["tx"], c["id"])


ADJ = [c for c in UP if c["ti"] == "f32" and c["to"] == "f32"]


@pytest.mark.parametrize("c", ADJ, ids=P.ids(ADJ))
def test_upsample_adjoint_identity(K, c):
    """<up(x), g> == <x, up_bwd(g)> in float64 from the kernels' own fp32 outputs: ties the forward to the backward.  Each side
    is a sum of n products of fp32 results carrying a few roundings each (4 products and 3 adds per bilinear output, twice
    that through the two backward passes and their candidate sums): 16 u (sum |up(x) g| + sum |x up_bwd(g)|)."""
    r = P.rng_of(dict(id=c["id"] + ":adjoint"))
    inp, _ = P.build(c)
    x = torch.from_numpy(inp["x"]).cuda()
    g = torch.from_numpy(r.standard_normal((c["N"],) + c["hout"] + (c["C"],), dtype=np.float32)).cuda()
    y = K.upsample_bilinear_ac(x, c["hout"], out_dtype=torch.float32, align_corners=c["align"])
    gx = K.upsample_bilinear_ac_bwd(g, c["hin"], out_dtype=torch.float32, align_corners=c["align"])
    lhs, rhs = (host(y) * host(g)), (host(x) * host(gx))
    bound = 16 * P.U * (np.abs(lhs).sum() + np.abs(rhs).sum())
    assert abs(lhs.sum() - rhs.sum()) <= bound, f"{c['id']}: <up x, g> = {lhs.sum()!r}, <x, up_bwd g> = {rhs.sum()!r}, bound {bound:.3e}"


# ---------------------------------------------------------------------------------------------------------------------- stem
SC = P.cases_of("stem_conv")


@pytest.mark.parametrize("c", SC, ids=P.ids(SC))
def test_stem_conv(K, c):
    inp, ref = P.build(c)
    y = K.stem_conv(torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["w"]).cuda(), DT[c["dt"]])
    reached(c)
    assert_close(host(y), ref["y"], c["dt"], c["id"])


SP = P.cases_of("stem_conv_pool")


@pytest.mark.parametrize("c", SP, ids=P.ids(SP))
def test_stem_conv_pool(K, c):
    inp, ref = P.build(c)
    cu = lambda v: torch.from_numpy(v).cuda()
    raw, act = K.stem_conv_pool(cu(inp["x"]), cu(inp["w"]), cu(inp["scale"]), cu(inp["shift"]))
    reached(c)
    assert_close(host(raw), ref["raw"], "bf16", f"{c['id']} raw")
    assert_close(host(act), ref["act"], "bf16", f"{c['id']} act")
