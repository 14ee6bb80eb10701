"""The bf16 NHWC BatchNorm kernels (csrc/bn_nhwc_core.h instantiated for bf16_t, through ops.bn_nhwc_fwd / ops.bn_nhwc_bwd on bf16 views) against float64 torch
BatchNorm on the bf16-rounded inputs.

Shapes: M in {1, 127, 128, 129, 2048, 2049} (the partial-block and finish-trip edges of the fp32 table) x C in {6, 8, 160}, and
C = 64 as slices of ld 72 at offset 8 (vector path) and of ld 65 (scalar path); one row per path whose work is just over
8192 * 256 items, so that the second grid-stride trip runs.  Flags: train / eval x relu x res; need_dx=False with dgamma only;
accumulate; out aliasing res.  Every row asserts the kernel it reached.

Bounds.  fp32 outputs (saved and running statistics, dgamma, dbeta): 1e-5 x max-abs of the reference.  bf16 outputs (y, dx):
|got - ref| <= 2^-8 |ref| + 1e-5 x max-abs -- one nearest-even rounding is <= 2^-9 relative, the other ulp lets the fp32 value sit
on the far side of a rounding boundary.  The backward reference takes its ReLU mask from the y handed to the kernel, so no element
is left out.  Reductions run twice for bit identity; a sliced `out` sits in a zeroed buffer that must stay zero around it.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
BF, F64 = torch.bfloat16, torch.float64
MS = (1, 127, 128, 129, 2048, 2049)
# (C, view): view = None (dense) or (element offset, ld) of a channel slice
LAYOUTS = ((6, None), (8, None), (160, None), (64, (8, 72)), (64, (0, 65)))
SHAPES = [(M, C, v) for M in MS for C, v in LAYOUTS]
BIG = {"vector": (262145, 64), "scalar": (349526, 6)}        # M * C / 8, resp. M * C, just over 8192 * 256


def sid(s):
    M, C, v = s
    return f"M{M}-C{C}" + ("" if v is None else f"-ld{v[1]}off{v[0]}")


def vec_of(C, view):
    return 8 if C % 8 == 0 and (view is None or (view[0] * 2 % 16 == 0 and view[1] * 2 % 16 == 0)) else 1


@pytest.fixture(scope="module")
def K():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    assert torch.cuda.is_available()
    return ops


def reached(name):
    from kdcc_amd import _lib
    got = _lib.last_plumbing_kernel()
    assert got == name, f"dispatched to {got}, this row is meant to cover {name}"


@functools.lru_cache(maxsize=None)
def data(M, C):
    """The bf16-rounded operands of one shape (CPU tensors; never modified) and their float64 values."""
    g = torch.Generator().manual_seed(1000 * C + M)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    d = dict(x=(r(C) * 2 + (0.5 + r(C).abs()) * r(M, C)).to(BF), gy=r(M, C).to(BF), res=r(M, C).to(BF),
             gamma=(1 + 0.5 * torch.rand(C, generator=g, dtype=F64)).float(), beta=(0.5 * r(C)).float(),
             rm=(0.3 * r(C)).float(), rv=(0.5 + torch.rand(C, generator=g, dtype=F64)).float())
    return d


@functools.lru_cache(maxsize=None)
def fwd_ref(M, C, train, relu):
    """float64: y, mean, invstd, running mean / var after the call."""
    d = data(M, C)
    x, gamma, beta = d["x"].to(F64), d["gamma"].to(F64), d["beta"].to(F64)
    rm, rv = d["rm"].to(F64).clone(), d["rv"].to(F64).clone()
    if train and M == 1:            # torch refuses one value per channel: mean = x, var = 0, and the running variance takes the biased 0
        mean, var = x[0].clone(), torch.zeros(C, dtype=F64)
        y = beta.expand(M, C).clone()
        rm, rv = (1 - MOM) * rm + MOM * mean, (1 - MOM) * rv
    else:
        y = F.batch_norm(x.t().reshape(1, C, M), rm, rv, gamma, beta, bool(train), MOM, EPS).reshape(C, M).t()
        mean, var = (x.mean(0), x.var(0, unbiased=False)) if train else (d["rm"].to(F64), d["rv"].to(F64))
    y = y.clamp_min(0) if relu else y
    return dict(y=y.contiguous(), mean=mean, invstd=(var + EPS).rsqrt(), rm=rm, rv=rv)


@functools.lru_cache(maxsize=None)
def bwd_ref(M, C, train, relu, with_res):
    """The operands handed to the backward (y, mean, invstd: the forward reference rounded to their storage types) and float64 dx,
    dgamma, dbeta of exactly those operands."""
    d, f = data(M, C), fwd_ref(M, C, train, relu)
    y, mean, invstd = f["y"].to(BF), f["mean"].float(), f["invstd"].float()
    g = d["gy"].to(F64)
    if relu:
        g = g * (y.to(F64) > 0)
    xhat = (d["x"].to(F64) - mean.to(F64)) * invstd.to(F64)
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    t = g - s1 / M - xhat * (s2 / M) if train else g
    dx = d["gamma"].to(F64) * invstd.to(F64) * t
    if with_res:
        dx = dx + d["res"].to(F64)
    return dict(y=y, mean=mean, invstd=invstd, dx=dx, dgamma=s2, dbeta=s1)


def place(a, view=None):
    """Device (1,1,M,C) view of the (M,C) tensor `a`; with view = (offset, ld): a channel slice of a wider zeroed buffer."""
    M, C = a.shape
    if view is None:
        return a.cuda().reshape(1, 1, M, C)
    off, ld = view
    buf = torch.zeros((1, 1, M, ld), dtype=a.dtype, device="cuda")
    buf[..., off:off + C] = a.cuda()
    return buf[..., off:off + C]


def out_place(M, C, view):
    """(view to write | None for a fresh tensor, whole buffer | None, offset)"""
    if view is None:
        return None, None, 0
    off, ld = view
    buf = torch.zeros((1, 1, M, ld), dtype=BF, device="cuda")
    return buf[..., off:off + C], buf, off


def stays_zero(buf, off, C, what):
    if buf is not None:
        assert not bool(buf[..., :off].any()) and not bool(buf[..., off + C:].any()), f"{what}: wrote outside the channel slice"


def close32(got, ref, what):
    got, ref = got.detach().cpu().to(F64).reshape(ref.shape), ref.to(F64)
    bound = 1e-5 * float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"ERR {what}: max |err| {err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(got).all() and err <= bound, f"{what}: |err| {err:.6e} > {bound:.6e}"


def close16(got, ref, what):
    assert got.dtype == BF, f"{what}: {got.dtype}"
    got, ref = got.detach().cpu().to(F64).reshape(ref.shape), ref.to(F64)
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * float(ref.abs().max())
    err = (got - ref).abs()
    print(f"ERR {what}: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3e}")
    assert torch.isfinite(got).all() and bool((err <= bound).all()), \
        f"{what}: {int((err > bound).sum())} of {err.numel()} elements miss, worst {float((err - bound).max()):.6e} over its bound"


def run_fwd(K, M, C, view, train, relu):
    d = data(M, C)
    x = place(d["x"], view)
    out, buf, off = out_place(M, C, view)
    rm, rv = d["rm"].cuda(), d["rv"].cuda()
    y, mean, invstd = K.bn_nhwc_fwd(x, d["gamma"].cuda(), d["beta"].cuda(), rm, rv, train, MOM, EPS, relu, out=out)
    reached(f"bn_lp_apply_kernel<{vec_of(C, view)}>")
    stays_zero(buf, off, C, "y")
    return y, mean, invstd, rm, rv


# ------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("relu", (False, True), ids=("plain", "relu"))
@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_forward(K, shape, train, relu):
    M, C, view = shape
    ref, d = fwd_ref(M, C, train, relu), data(M, C)
    y, mean, invstd, rm, rv = run_fwd(K, M, C, view, train, relu)
    what = f"{sid(shape)} {'train' if train else 'eval'}{' relu' if relu else ''}"
    assert y.dtype == BF and mean.dtype == invstd.dtype == torch.float32
    close16(y, ref["y"], what + " y")
    close32(mean, ref["mean"], what + " save_mean")
    close32(invstd, ref["invstd"], what + " save_invstd")
    if train:
        close32(rm, ref["rm"], what + " running_mean")
        close32(rv, ref["rv"], what + " running_var")
    else:
        assert torch.equal(rm.cpu(), d["rm"]) and torch.equal(rv.cpu(), d["rv"]), "eval mode wrote the running statistics"
        assert torch.equal(mean.cpu(), d["rm"]), "eval mode saves the running mean as it is"
    y2, mean2, invstd2, rm2, rv2 = run_fwd(K, M, C, view, train, relu)
    assert all(torch.equal(a, b) for a, b in ((y, y2), (mean, mean2), (invstd, invstd2), (rm, rm2), (rv, rv2))), "not bit-reproducible"


def test_forward_running_statistics_are_optional(K):
    M, C = 129, 8
    d, ref = data(M, C), fwd_ref(M, C, True, False)
    y, mean, invstd = K.bn_nhwc_fwd(place(d["x"]), d["gamma"].cuda(), d["beta"].cuda(), None, None, True, MOM, EPS)
    close16(y, ref["y"], "no running statistics: y")
    close32(mean, ref["mean"], "no running statistics: save_mean")


# ------------------------------------------------------------------------------------------------------------------ backward
def run_bwd(K, M, C, view, train, relu, with_res, **kw):
    d, ref = data(M, C), bwd_ref(M, C, train, relu, with_res)
    gy, x, y = place(d["gy"], view), place(d["x"], view), place(ref["y"], view)
    res = place(d["res"], view) if with_res else None
    out, buf, off = out_place(M, C, view)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dx = K.bn_nhwc_bwd(gy, x, y, d["gamma"].cuda(), ref["mean"].cuda(), ref["invstd"].cuda(), train, relu, res=res, dgamma=dg, dbeta=db,
                       out=out, **kw)
    reached(f"bn_lp_dx_kernel<{vec_of(C, view)}>")
    stays_zero(buf, off, C, "dx")
    return dx, dg, db


@pytest.mark.parametrize("with_res", (False, True), ids=("nores", "res"))
@pytest.mark.parametrize("relu", (False, True), ids=("plain", "relu"))
@pytest.mark.parametrize("train", (True, False), ids=("train", "eval"))
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_backward(K, shape, train, relu, with_res):
    M, C, view = shape
    ref = bwd_ref(M, C, train, relu, with_res)
    what = f"{sid(shape)} {'train' if train else 'eval'}{' relu' if relu else ''}{' res' if with_res else ''}"
    if relu and M * C >= 64:
        assert 0.05 < float((ref["y"].float() > 0).float().mean()) < 0.95, "the ReLU mask is one-sided"
    dx, dg, db = run_bwd(K, M, C, view, train, relu, with_res)
    close16(dx, ref["dx"], what + " dx")
    close32(dg, ref["dgamma"], what + " dgamma")
    close32(db, ref["dbeta"], what + " dbeta")
    dx2, dg2, db2 = run_bwd(K, M, C, view, train, relu, with_res)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2), "not bit-reproducible"


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: sid((2049,) + l))
def test_backward_parameter_gradients_only(K, layout):
    """need_dx=False with dgamma alone: the reduction runs, no dx is made, dbeta is not asked for."""
    (C, view), M = layout, 2049
    d, ref = data(M, C), bwd_ref(M, C, True, True, False)
    dg = torch.empty(C, device="cuda")
    dx = K.bn_nhwc_bwd(place(d["gy"], view), place(d["x"], view), place(ref["y"], view), d["gamma"].cuda(), ref["mean"].cuda(),
                       ref["invstd"].cuda(), True, True, need_dx=False, dgamma=dg)
    reached(f"bn_lp_grad_partial_kernel<{vec_of(C, view)}>")
    assert dx is None
    close32(dg, ref["dgamma"], f"C{C} dgamma only")


@pytest.mark.parametrize("layout", ((6, None), (160, None)), ids=("C6", "C160"))
def test_backward_accumulate(K, layout):
    (C, view), M = layout, 2049
    d, ref = data(M, C), bwd_ref(M, C, True, True, True)
    g = torch.Generator().manual_seed(C)
    dg0, db0 = torch.randn(C, generator=g) * 30, torch.randn(C, generator=g) * 30
    dg, db = dg0.cuda(), db0.cuda()
    dx = K.bn_nhwc_bwd(place(d["gy"]), place(d["x"]), place(ref["y"]), d["gamma"].cuda(), ref["mean"].cuda(), ref["invstd"].cuda(), True, True,
                       res=place(d["res"]), dgamma=dg, dbeta=db, accumulate=True)
    close16(dx, ref["dx"], f"C{C} accumulate dx")
    close32(dg, dg0.to(F64) + ref["dgamma"], f"C{C} dgamma +=")
    close32(db, db0.to(F64) + ref["dbeta"], f"C{C} dbeta +=")


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: sid((2049,) + l))
def test_backward_out_aliasing_res(K, layout):
    """dx accumulates in place into the gradient it is added to: the same bits as into a tensor of its own."""
    (C, view), M = layout, 2049
    d, ref = data(M, C), bwd_ref(M, C, True, True, True)
    args = lambda: (place(d["gy"], view), place(d["x"], view), place(ref["y"], view), d["gamma"].cuda(), ref["mean"].cuda(), ref["invstd"].cuda(),
                    True, True)
    res = place(d["res"], view)
    apart = K.bn_nhwc_bwd(*args(), res=res)
    same = K.bn_nhwc_bwd(*args(), res=res, out=res)
    reached(f"bn_lp_dx_kernel<{vec_of(C, view)}>")
    assert same.data_ptr() == res.data_ptr() and torch.equal(same, apart)
    close16(same, ref["dx"], f"C{C} dx into res")


# ------------------------------------------------------------------------------------- the second grid-stride trip of each path
@pytest.mark.parametrize("path", sorted(BIG))
def test_the_second_grid_stride_trip(K, path):
    """Work just over 8192 * 256 items: blocks of the capped grid come round again.  y and dx only (train, relu, res)."""
    M, C = BIG[path]
    v = vec_of(C, None)
    assert (path == "vector") == (v == 8) and 8192 * 256 < M * C // v <= 8192 * 256 + 8
    d, f, b = data(M, C), fwd_ref(M, C, True, True), bwd_ref(M, C, True, True, True)
    y, _, _ = K.bn_nhwc_fwd(place(d["x"]), d["gamma"].cuda(), d["beta"].cuda(), None, None, True, MOM, EPS, True)
    reached(f"bn_lp_apply_kernel<{v}>")
    close16(y, f["y"], f"{path} over the cap: y")
    dx = K.bn_nhwc_bwd(place(d["gy"]), place(d["x"]), place(b["y"]), d["gamma"].cuda(), b["mean"].cuda(), b["invstd"].cuda(), True, True,
                       res=place(d["res"]))
    reached(f"bn_lp_dx_kernel<{v}>")
    close16(dx, b["dx"], f"{path} over the cap: dx")
    for cache in (data, fwd_ref, bwd_ref):      # (the big operands are used here only)
        cache.cache_clear()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_and_launch_nothing(K):
    from kdcc_amd import _lib
    M, C = 128, 8
    d, ref = data(M, C), bwd_ref(M, C, True, True, True)
    gamma, beta, mean, invstd = d["gamma"].cuda(), d["beta"].cuda(), ref["mean"].cuda(), ref["invstd"].cuda()
    x, gy, y, res = place(d["x"]), place(d["gy"]), place(ref["y"]), place(d["res"])
    K.bn_nhwc_fwd(x.float(), gamma, beta, None, None, True, MOM, EPS)           # the fp32 twin: the note the refusals must leave alone
    last = _lib.last_plumbing_kernel()
    assert last == "bn_nhwc_apply_kernel<4>"
    out = torch.full((1, 1, M, C), 3.0, dtype=BF, device="cuda")
    keep = out.clone()
    with pytest.raises(ValueError, match="mixed dtype"):
        K.bn_nhwc_fwd(x, gamma, beta, None, None, True, MOM, EPS, out=out.float())
    with pytest.raises(ValueError, match="mixed dtype"):
        K.bn_nhwc_fwd(x.float(), gamma, beta, None, None, True, MOM, EPS, out=out)
    for bad in ("gy", "y", "res", "out"):
        ops_ = dict(gy=gy, y=y, res=res, out=out)
        ops_[bad] = ops_[bad].float()
        with pytest.raises(ValueError, match="mixed dtype"):
            K.bn_nhwc_bwd(ops_["gy"], x, ops_["y"], gamma, mean, invstd, True, True, res=ops_["res"], out=ops_["out"])
    with pytest.raises(TypeError):
        K.bn_nhwc_fwd(x.half(), gamma, beta, None, None, True, MOM, EPS)
    with pytest.raises(ValueError):                                             # the per-channel vectors stay fp32
        K.bn_nhwc_fwd(x, gamma.to(BF), beta, None, None, True, MOM, EPS)
    with pytest.raises(_lib.KdccError):                                         # a host tensor
        K.bn_nhwc_fwd(x.cpu(), gamma, beta, None, None, True, MOM, EPS)
    with pytest.raises(_lib.KdccError):
        K.bn_nhwc_bwd(gy.cpu(), x, y, gamma, mean, invstd, True, True)
    # illegal overlaps of out: an operand other than res; res one pixel on (element sizes decide: 2 bytes an element)
    for clash in (gy, x, y):
        with pytest.raises(ValueError, match="overlaps"):
            K.bn_nhwc_bwd(gy, x, y, gamma, mean, invstd, True, True, out=clash)
    wide = torch.zeros((1, 1, M + 1, C), dtype=BF, device="cuda")
    with pytest.raises(ValueError, match="overlaps"):
        K.bn_nhwc_bwd(gy, x, y, gamma, mean, invstd, True, True, res=wide[:, :, 1:], out=wide[:, :, :M])
    # ... and what lies just behind out's last byte is no overlap
    two = torch.zeros((1, 1, 2 * M, C), dtype=BF, device="cuda")
    two[:, :, M:] = res
    assert _lib.last_plumbing_kernel() == last and torch.equal(out, keep) and not bool(wide.any()), "a refused call launched something"
    dx = K.bn_nhwc_bwd(gy, x, y, gamma, mean, invstd, True, True, res=two[:, :, M:], out=two[:, :, :M])
    close16(dx, ref["dx"], "out next to res")
    assert torch.equal(two[:, :, M:], res)


# ------------------------------------------------------------------------------------------- one implementation, two storages
def test_fp32_and_bf16_storage_are_one_implementation(K):
    """The same bf16-representable values through the fp32 and the bf16 entry points: (N, H, W, C) = (2, 9, 15, 20), M = 270 -- three
    stage-1 row blocks, the last of 14 rows; C = 20 puts fp32 on the float4 elementwise kernels, bf16 on the scalar ones throughout
    and both storages on the scalar partials.  The reductions are the same kernels on the same values: every fp32 vector bit for bit; the
    elementwise outputs differ by the one rounding of the bf16 store."""
    N, H, W, C = 2, 9, 15, 20
    g = torch.Generator().manual_seed(20270)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x16, gy16, res16 = ((r(C) + (0.5 + r(C).abs()) * r(N, H, W, C)).to(BF).cuda(), r(N, H, W, C).to(BF).cuda(), r(N, H, W, C).to(BF).cuda())
    gamma, beta = (1 + 0.5 * torch.rand(C, generator=g, dtype=F64)).float().cuda(), (0.5 * r(C)).float().cuda()
    rm0, rv0 = (0.3 * r(C)).float().cuda(), (0.5 + torch.rand(C, generator=g, dtype=F64)).float().cuda()
    fwd = {}
    for dt, name in ((BF, "bn_lp_apply_kernel<1>"), (torch.float32, "bn_nhwc_apply_kernel<4>")):
        rm, rv = rm0.clone(), rv0.clone()
        y, mean, invstd = K.bn_nhwc_fwd(x16.to(dt), gamma, beta, rm, rv, True, MOM, EPS, True)
        reached(name)
        fwd[dt] = dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv)
    a, b = fwd[BF], fwd[torch.float32]
    for k in ("mean", "invstd", "rm", "rv"):
        assert torch.equal(a[k], b[k]), f"forward {k}: the two storages disagree"
    assert not torch.equal(a["rm"], rm0) and not torch.equal(a["rv"], rv0)
    assert a["y"].dtype == BF and torch.equal(a["y"], b["y"].to(BF)), "forward y"
    assert 0.05 < float((a["y"] > 0).float().mean()) < 0.95, "the ReLU mask is one-sided"
    bwd = {}
    for dt, name in ((BF, "bn_lp_dx_kernel<1>"), (torch.float32, "bn_nhwc_dx_kernel<4>")):
        dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        dx = K.bn_nhwc_bwd(gy16.to(dt), x16.to(dt), a["y"].to(dt), gamma, a["mean"], a["invstd"], True, True, res=res16.to(dt), dgamma=dg, dbeta=db)
        reached(name)
        bwd[dt] = dict(dx=dx, dgamma=dg, dbeta=db)
    a, b = bwd[BF], bwd[torch.float32]
    assert torch.equal(a["dgamma"], b["dgamma"]) and torch.equal(a["dbeta"], b["dbeta"]), "backward dgamma / dbeta"
    assert a["dx"].dtype == BF and torch.equal(a["dx"], b["dx"].to(BF)), "backward dx"
