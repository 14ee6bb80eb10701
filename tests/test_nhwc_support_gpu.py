"""Every branch and loop trip of the fp32 NHWC kernels behind the classification models and the HRNet-OCR head
(csrc/hrnet_ops.hip, bn_nhwc.hip with bn_nhwc_core.h and bn_select.h, dense_ops.hip) against float64 on the CPU, element by element against the
per-element bounds of tests/_nhwc_support_cases.py (derived there from each kernel's reduction plan).

Each row asserts the kernel it reached where the entry point chooses one, compares every output with its bound (a bound of 0:
bit for bit), prints max(err / bound) per output, hands every entry point that takes `out=` a slice of a sentinel-filled wider
buffer where the row says so and checks the sentinel afterwards, and runs reductions twice for bit identity.

The 181 tests of this file take about 5 s together on an MI355X; the slowest (the 16400 x 512 backward row) 0.7 s.
"""
import numpy as np
import pytest
import torch

import _nhwc_support_cases as S

pytestmark = pytest.mark.gpu

SENT = 7.0


@pytest.fixture(scope="module")
def K():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    assert torch.cuda.is_available()
    return ops


def reached(c):
    from kdcc_amd import _lib
    if c["kernel"]:
        got = _lib.last_plumbing_kernel()
        assert got == c["kernel"], f"{c['id']}: dispatched to {got}, this row is meant to cover {c['kernel']}"


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def place(a, view=None):
    """Device tensor of `a`; with view = (float offset, ld): a channel slice of a wider sentinel-filled buffer."""
    t = cu(a)
    if view is None:
        return t
    off, ld = view
    buf = torch.full(t.shape[:-1] + (ld,), SENT, device="cuda")
    buf[..., off:off + t.shape[-1]] = t
    return buf[..., off:off + t.shape[-1]]


def out_place(shape, view=None):
    """(view to write, whole buffer, offset): the buffer outside the view must keep its sentinel."""
    if view is None:
        t = torch.full(tuple(shape), SENT, device="cuda")
        return t, None, 0
    off, ld = view
    buf = torch.full(tuple(shape[:-1]) + (ld,), SENT, device="cuda")
    return buf[..., off:off + shape[-1]], buf, off


def untouched(v, buf, off, what):
    if buf is not None:
        C = v.shape[-1]
        assert bool((buf[..., :off] == SENT).all()) and bool((buf[..., off + C:] == SENT).all()), f"{what}: wrote outside the channel slice"


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def within(got, ref, bound, what):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape}, reference {ref.shape}"
    bound = np.asarray(bound, np.float64) + np.zeros_like(ref)
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    print(f"RATIO {what}: max err/bound {ratio.max() if ratio.size else 0.0:.3e}")
    assert np.isfinite(got).all(), f"{what}: not finite"
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (f"{what}: |err| {err.flat[worst]:.6e} > bound {bound.flat[worst]:.6e} at {np.unravel_index(worst, ref.shape)} "
                                  f"(got {got.flat[worst]!r}, ref {ref.flat[worst]!r}); {int((err > bound).sum())} of {err.size} elements miss")


def compare(c, ref, got):
    for name, r, b in S.checks(c, ref):
        within(host(got[name]), r, b, f"{c['id']} {name}")


# ---------------------------------------------------------------------------------------------------------------------- OCR
OG = S.cases_of("ocr_gather")


@pytest.mark.parametrize("c", OG, ids=S.ids(OG))
def test_ocr_gather(K, c):
    inp, ref = S.build(c)
    lg, f = place(inp["logits"], c["views"].get("logits")), place(inp["feats"], c["views"].get("feats"))
    ctx, mx, lse = K.ocr_gather(lg, f)
    compare(c, ref, dict(ctx=ctx, mx=mx, lse=lse))
    ctx2, mx2, lse2 = K.ocr_gather(lg, f)
    assert torch.equal(ctx, ctx2) and torch.equal(mx, mx2) and torch.equal(lse, lse2), "not bit-reproducible"


OGB = S.cases_of("ocr_gather_bwd")


@pytest.mark.parametrize("c", OGB, ids=S.ids(OGB))
def test_ocr_gather_bwd(K, c):
    inp, ref = S.build(c)
    lg, f = place(inp["logits"], c["views"].get("logits")), place(inp["feats"], c["views"].get("feats"))
    df, dl = K.ocr_gather_bwd(cu(inp["gctx"]), cu(inp["ctx"]), lg, f, cu(inp["lse"]))
    compare(c, ref, dict(d_feats=df, d_logits=dl))


OA = S.cases_of("ocr_attend")


@pytest.mark.parametrize("c", OA, ids=S.ids(OA))
def test_ocr_attend(K, c):
    inp, ref = S.build(c)
    ctx = K.ocr_attend(place(inp["query"], c["views"].get("query")), cu(inp["key"]), cu(inp["value"]), scale=c["flags"].get("scale"))
    compare(c, ref, dict(ctx=ctx))


OAB = S.cases_of("ocr_attend_bwd")


@pytest.mark.parametrize("c", OAB, ids=S.ids(OAB))
def test_ocr_attend_bwd(K, c):
    inp, ref = S.build(c)
    args = (place(inp["g"], c["views"].get("g")), place(inp["query"], c["views"].get("query")), cu(inp["key"]), cu(inp["value"]))
    dq, dk, dv = K.ocr_attend_bwd(*args, scale=c["flags"].get("scale"))
    compare(c, ref, dict(d_query=dq, d_key=dk, d_value=dv))
    dq2, dk2, dv2 = K.ocr_attend_bwd(*args, scale=c["flags"].get("scale"))
    assert torch.equal(dk, dk2) and torch.equal(dv, dv2) and torch.equal(dq, dq2), "not bit-reproducible"


@pytest.mark.parametrize("op, shape", S.REFUSALS, ids=[f"{op}-K{s[2]}-C{s[3]}" for op, s in S.REFUSALS])
def test_ocr_refuses_what_does_not_fit_the_lds(K, op, shape):
    from kdcc_amd import _lib
    N, HW, Kk, C = shape
    r = np.random.default_rng(5)
    f = lambda *s: cu(r.standard_normal(s))
    if op == "ocr_gather_bwd":
        lg, feats = f(N, HW, Kk), f(N, HW, C)
        ctx, mx, lse = K.ocr_gather(lg, feats)                      # the forward stages no K x C panel and accepts the shape
        assert bool(torch.isfinite(ctx).all())
        with pytest.raises(_lib.KdccError, match="64 KiB"):
            K.ocr_gather_bwd(f(N, Kk, C), ctx, lg, feats, lse)
    else:
        with pytest.raises(_lib.KdccError, match="64 KiB"):
            K.ocr_attend(f(N, HW, C), f(N, Kk, C), f(N, Kk, C))
        with pytest.raises(_lib.KdccError, match="64 KiB"):
            K.ocr_attend_bwd(f(N, HW, C), f(N, HW, C), f(N, Kk, C), f(N, Kk, C))


# --------------------------------------------------------------------------------------------------------------- HRNet fuse
HF = S.cases_of("hr_fuse")


@pytest.mark.parametrize("c", HF, ids=S.ids(HF))
def test_hr_fuse(K, c):
    inp, ref = S.build(c)
    N, Ho, Wo, C = c["shape"]
    view = c["views"].get("all")
    srcs = [place(s, view) for s in inp["srcs"]]
    out, buf, off = out_place(c["shape"], view)
    if c["flags"].get("size"):
        y = K.hr_fuse(srcs, size=(Ho, Wo))
    else:
        y = K.hr_fuse(srcs, out=out)
        untouched(out, buf, off, c["id"])
    compare(c, ref, dict(y=y))


HFB = S.cases_of("hr_fuse_bwd")


@pytest.mark.parametrize("c", HFB, ids=S.ids(HFB))
def test_hr_fuse_bwd(K, c):
    from kdcc_amd import _lib
    inp, ref = S.build(c)
    N, Ho, Wo, C = c["shape"]
    view = c["views"].get("all")
    gy, y = place(inp["gy"], view), place(inp["y"], view)
    need = c["flags"].get("need")
    if view is None:
        outs = K.hr_fuse_bwd(gy, y, c["srcs"], need=need)
    else:      # every gradient a slice of a wider buffer: the entry point itself (ops.hr_fuse_bwd allocates dense ones)
        places = [out_place((N, h, w, C), view) for h, w in c["srcs"]]
        outs = [p[0] for p in places]
        arr = K._hr_views(outs, (N, C), "hr_fuse_bwd")
        _lib.check(_lib.lib().kd_hr_fuse_bwd(K._ptr(gy), K._pixel_ld(gy), K._ptr(y), K._pixel_ld(y), arr, len(outs), N, Ho, Wo, C, K.stream_ptr()),
                   "kd_hr_fuse_bwd")
        for v, buf, off in places:
            untouched(v, buf, off, c["id"])
    for i, nd in enumerate(need or ()):
        assert (outs[i] is not None) == bool(nd)
    compare(c, ref, {f"gsrc{i}": o for i, o in enumerate(outs) if o is not None})


# ----------------------------------------------------------------------------------------------------------------------- BN
def _bn_x(c, inp, name="x"):
    M, C = c["M"], c["C"]
    return place(inp[name].reshape(1, 1, M, C), c["views"].get(name))


def _running(c, inp):
    run = c["flags"].get("run", "both")
    return (cu(inp["run_mean"]) if run in ("mean", "both") else None), (cu(inp["run_var"]) if run in ("var", "both") else None)


def _compare_bn_fwd(c, inp, ref, y, rm, rv, extra):
    M, C = c["M"], c["C"]
    got = dict(y=y.reshape(M, C), **extra)
    names = [n for n in S.outputs_of(c) if not (n == "run_mean" and rm is None) and not (n == "run_var" and rv is None)]
    if rm is not None:
        got["run_mean"] = rm
    if rv is not None:
        got["run_var"] = rv
    for name in names:
        within(host(got[name]), ref[name], ref["bounds"][name], f"{c['id']} {name}")
    if not c["train"]:     # eval mode leaves the running statistics alone
        assert torch.equal(rm, cu(inp["run_mean"])) and torch.equal(rv, cu(inp["run_var"]))


BF = S.cases_of("bn_fwd")


@pytest.mark.parametrize("c", BF, ids=S.ids(BF))
def test_bn_nhwc_fwd(K, c):
    inp, ref = S.build(c)
    M, C = c["M"], c["C"]
    x = _bn_x(c, inp)
    rm, rv = _running(c, inp)
    out, buf, off = out_place((1, 1, M, C), c["views"].get("y"))
    g, b = cu(inp["gamma"]), cu(inp["beta"])
    y, mean, invstd = K.bn_nhwc_fwd(x, g, b, rm, rv, c["train"], S.BN_MOM, S.BN_EPS, relu=c["relu"], out=out)
    reached(c)
    untouched(out, buf, off, c["id"])
    _compare_bn_fwd(c, inp, ref, y, rm, rv, dict(mean=mean, invstd=invstd))
    if c["train"]:
        y2, mean2, invstd2 = K.bn_nhwc_fwd(x, g, b, None, None, True, S.BN_MOM, S.BN_EPS, relu=c["relu"])
        assert torch.equal(mean, mean2) and torch.equal(invstd, invstd2) and torch.equal(y2.reshape(M, C), y.reshape(M, C)), "not bit-reproducible"


BS = S.cases_of("bn_stats")


@pytest.mark.parametrize("c", BS, ids=S.ids(BS))
def test_bn_nhwc_stats(K, c):
    inp, ref = S.build(c)
    x = _bn_x(c, inp)
    mean, invstd, vu = K.bn_nhwc_stats(x, S.BN_EPS)
    compare(c, ref, dict(mean=mean, invstd=invstd, var_unb=vu))
    m2, i2, v2 = K.bn_nhwc_stats(x, S.BN_EPS)
    assert torch.equal(mean, m2) and torch.equal(invstd, i2) and torch.equal(vu, v2), "not bit-reproducible"
    # per channel the bits kd_bn_nhwc_fwd saves
    _, m3, i3 = K.bn_nhwc_fwd(x, cu(inp["gamma"]), cu(inp["beta"]), None, None, True, S.BN_MOM, S.BN_EPS)
    assert torch.equal(mean, m3) and torch.equal(invstd, i3)


BA = S.cases_of("bn_apply")


@pytest.mark.parametrize("c", BA, ids=S.ids(BA))
def test_bn_nhwc_apply(K, c):
    inp, ref = S.build(c)
    M, C = c["M"], c["C"]
    x = _bn_x(c, inp)
    rm, rv = _running(c, inp)
    out, buf, off = out_place((1, 1, M, C), c["views"].get("y"))
    y = K.bn_nhwc_apply(x, cu(inp["gamma"]), cu(inp["beta"]), cu(inp["mean"]), cu(inp["invstd"]), cu(inp["var_unb"]), rm, rv, S.BN_MOM,
                        relu=c["relu"], out=out)
    reached(c)
    untouched(out, buf, off, c["id"])
    _compare_bn_fwd(c, inp, ref, y, rm, rv, {})


BB = S.cases_of("bn_bwd")


@pytest.mark.parametrize("c", BB, ids=S.ids(BB))
def test_bn_nhwc_bwd(K, c):
    inp, ref = S.build(c)
    M, C, fl = c["M"], c["C"], c["flags"]
    gy, x, y = _bn_x(c, inp, "gy"), _bn_x(c, inp), _bn_x(c, inp, "y")
    res = _bn_x(c, inp, "res") if fl.get("res") else None
    need_dx = fl.get("need_dx", True)
    want = S.outputs_of(c)
    out, buf, off = (res, None, 0) if fl.get("alias") else out_place((1, 1, M, C), c["views"].get("dx")) if need_dx else (None, None, 0)
    vec = lambda name: (cu(inp[name + "0"]) if fl.get("accumulate") else torch.full((C,), SENT, device="cuda")) if name in want else None
    dg, db = vec("dgamma"), vec("dbeta")
    args = (gy, x, y, cu(inp["gamma"]), cu(inp["mean"]), cu(inp["invstd"]), c["train"])
    dx = K.bn_nhwc_bwd(*args, relu=c["relu"], res=res, need_dx=need_dx, dgamma=dg, dbeta=db, accumulate=bool(fl.get("accumulate")), out=out)
    reached(c)
    assert (dx is not None) == need_dx
    if need_dx:
        untouched(out, buf, off, c["id"])
    got = dict(dgamma=dg, dbeta=db)
    if need_dx:
        got["dx"] = dx.reshape(M, C)
    for name in want:
        within(host(got[name]), ref[name], ref["bounds"][name], f"{c['id']} {name}")
    if "dgamma" in want and not fl.get("accumulate") and not fl.get("alias"):
        dg2 = torch.full((C,), SENT, device="cuda")
        K.bn_nhwc_bwd(*args, relu=c["relu"], need_dx=False, dgamma=dg2)
        assert torch.equal(dg, dg2), "not bit-reproducible"


# --------------------------------------------------------------------------------------------------------------------- pool
AP = S.cases_of("avgpool")


@pytest.mark.parametrize("c", AP, ids=S.ids(AP))
def test_avgpool2x2(K, c):
    inp, ref = S.build(c)
    N, H, W, C = c["shape"]
    out, buf, off = out_place((N, H // 2, W // 2, C), c["views"].get("y"))
    y = K.avgpool2x2(place(inp["x"], c["views"].get("x")), out=out)
    reached(c)
    untouched(out, buf, off, c["id"])
    compare(c, ref, dict(y=y))


APB = S.cases_of("avgpool_bwd")


@pytest.mark.parametrize("c", APB, ids=S.ids(APB))
def test_avgpool2x2_bwd(K, c):
    inp, ref = S.build(c)
    N, H, W, C = c["shape"]
    out, buf, off = out_place(c["shape"], c["views"].get("gx"))
    gx = K.avgpool2x2_bwd(place(inp["gy"], c["views"].get("gy")), (H, W), out=out)
    reached(c)
    untouched(out, buf, off, c["id"])
    compare(c, ref, dict(gx=gx))
