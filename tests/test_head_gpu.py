"""kd_head_bn_relu_pool_fwd / _bwd (csrc/head_ops.hip) against float64 on the CPU, evaluated on the operands as stored
(tests/_headref.py): every channel count, batch, map size, layout and mode of CASES, the kernel each call reached
(kd_debug_last_plumbing_kernel against the restated selector), the sentinel bytes around channel slices, and two calls bit for bit.

The error bars are derived, not tuned.  With u = 2^-24 and A = |xhat gamma| + |beta| per element, fp32 evaluation of
y = (x - mean) invstd gamma + beta is off by at most 4 u A (a subtraction, two products, an addition); a sum of n terms in ANY
order by at most (n - 1) u sum |terms| (the recursive-summation bound) on top of the terms' own errors:
  pooled   (HW + 8) u mean_p A                        (HW - 1 additions, the division, 4 u A per term, second-order slack)
  dbeta    (M + 2) u sum |g'|                         (g' = gpooled / HW: one rounding per term)
  dgamma   (M + 4) u sum |g' xhat|                    (g', xhat (2 u) and their product)
  dx       |k| ((B_dbeta + |xhat| B_dgamma) / M + 8 u (|g'| + |dbeta / M| + |xhat dgamma / M|)) + 2 u |dx|  in train mode,
           4 u |dx| in eval mode                      (k = gamma invstd)
The backward's ReLU mask is discontinuous, so the inputs are built with no activation closer to zero than 16 u A: there fp32 and
float64 agree on every sign, and the bars above hold.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _headref as R  # noqa: E402

U = 2.0 ** -24
SENTINEL = 12345.0
SHAPES = {64: (8, 8), 35: (5, 7), 1: (1, 1)}
LAYOUTS = {"dense": (0, 0), "slice4": (4, 8), "slice1": (1, 8)}        # channel offset of the slice, extra channels of the buffer
CASES = [dict(C=C, N=N, HW=HW, layout=lay, training=tr, shift=0.0)
         for C, N, HW, lay, tr in itertools.product((256, 64, 20, 4), (3, 1), (64, 35, 1), LAYOUTS, (True, False))]
CASES += [dict(C=64, N=3, HW=64, layout=lay, training=tr, shift=1e3) for lay in ("dense", "slice1") for tr in (True, False)]
assert len(CASES) == 4 * 2 * 3 * 3 * 2 + 4
ids = lambda cs: [f"C{c['C']}-N{c['N']}-HW{c['HW']}-{c['layout']}-{'train' if c['training'] else 'eval'}" + ("-shift" if c["shift"] else "")
                  for c in cs]


def _operands(c):
    """(x, gamma, beta, mean, invstd, gpooled) fp32 on the host; the last channel's activations are all negative; no activation
    within 16 u A of zero (see the module docstring)."""
    C, N, (H, W) = c["C"], c["N"], SHAPES[c["HW"]]
    g = torch.Generator().manual_seed(1000 * C + 100 * N + c["HW"] + (7 if c["training"] else 0))
    x = torch.randn((N, H, W, C), generator=g) * 1.5 + torch.randn(C, generator=g) + c["shift"]
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1                                  # (a negative gamma flips which side of the mean is active)
    beta = torch.randn(C, generator=g) * 0.3
    beta[C - 1] = -60.0                               # |xhat gamma| stays far below: the channel is dead everywhere
    gp = torch.randn((N, C), generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.2 + c["shift"], torch.rand(C, generator=g) + 0.5
    for _ in range(8):
        if c["training"] and N * H * W > 1:
            xd = x.double()
            mean = xd.mean(dim=(0, 1, 2)).float()
            invstd = (1.0 / torch.sqrt(xd.var(dim=(0, 1, 2), unbiased=False) + 1e-5)).float()
        elif c["training"]:                           # (one pixel: the batch variance is 0)
            mean, invstd = x.reshape(C).clone(), torch.full((C,), 1.0 / 1e-5 ** 0.5)
        else:
            mean, invstd = rm, (1.0 / torch.sqrt(rv.double() + 1e-5)).float()
        xhat = (x.double() - mean.double()) * invstd.double()
        y = xhat * gamma.double() + beta.double()
        close = y.abs() <= 16 * U * ((xhat * gamma.double()).abs() + beta.double().abs())
        if not bool(close.any()):
            break
        x = torch.where(close, x + 0.25, x)
    assert not bool(close.any()), "an activation too close to zero for its sign to be certain in fp32"
    assert bool((y[..., C - 1] < -1).all())
    return x, gamma, beta, mean, invstd, gp


def _place(t, layout, fill=True):
    """The (N,H,W,C) device view of `layout` holding t (or uninitialised), and the buffer it is a slice of."""
    off, extra = LAYOUTS[layout]
    N, H, W, C = t.shape
    wide = torch.full((N, H, W, C + extra), SENTINEL, device="cuda")
    view = wide[..., off:off + C] if extra else wide
    if fill:
        view.copy_(t.cuda())
    return view, wide


def _outside_untouched(wide, layout, C):
    off, extra = LAYOUTS[layout]
    if not extra:
        return True
    return bool((wide[..., :off] == SENTINEL).all()) and bool((wide[..., off + C:] == SENTINEL).all())


def _within(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    worst = float((err - bound).max())
    assert worst <= 0, f"{what}: error exceeds its bound by {worst:.3e} (max error {float(err.max()):.3e}, max bound {float(bound.max()):.3e})"
    return 1


def _run(c):
    """Both entry points on one case; returns the number of comparisons made."""
    from kdcc_amd import _lib, ops
    C, N, HW, lay, training = c["C"], c["N"], c["HW"], c["layout"], c["training"]
    M = N * HW
    x, gamma, beta, mean, invstd, gp = _operands(c)
    p_r, dx_r, dg_r, db_r, y = R.head_ref(x, gamma, beta, mean, invstd, gp, training)
    xhat = (x.double() - mean.double()) * invstd.double()
    A = (xhat * gamma.double()).abs() + beta.double().abs()
    xv, xw = _place(x, lay)
    dev = [t.cuda() for t in (gamma, beta, mean, invstd)]
    done = 0
    # ---- forward
    pooled = ops.head_bn_relu_pool_fwd(xv, *dev)
    assert _lib.last_plumbing_kernel() == R.predict(False, C, xv.data_ptr(), xv.stride(2))[0]
    done += _within(pooled, p_r, (HW + 8) * U * A.mean(dim=(1, 2)), "pooled")
    assert torch.equal(pooled, ops.head_bn_relu_pool_fwd(xv, *dev)), "two forward calls differ"
    assert bool((pooled[:, C - 1] == 0).all())
    # ---- backward, dx into a view of the same layout
    dxv, dxw = _place(x, lay, fill=False)
    gpd = gp.cuda()
    dx, dg, db = ops.head_bn_relu_pool_bwd(xv, gpd, *dev, training, out=dxv)
    name, vec, grid = R.predict(True, C, xv.data_ptr(), xv.stride(2), dxv.data_ptr(), dxv.stride(2))
    assert _lib.last_plumbing_kernel() == name and (vec == 4) == (lay != "slice1" and C % 4 == 0)
    gq = torch.where(y > 0, (gp.double() / HW).view(N, 1, 1, C).expand_as(y), torch.zeros_like(y))
    B_db = (M + 2) * U * gq.abs().sum(dim=(0, 1, 2))
    B_dg = (M + 4) * U * (gq * xhat).abs().sum(dim=(0, 1, 2))
    done += _within(db, db_r, B_db, "dbeta")
    done += _within(dg, dg_r, B_dg, "dgamma")
    k = (gamma.double() * invstd.double()).abs()
    if training:
        B_dx = k * ((B_db + xhat.abs() * B_dg) / M + 8 * U * (gq.abs() + (db_r / M).abs() + (xhat * dg_r / M).abs())) + 2 * U * dx_r.abs()
    else:
        B_dx = 4 * U * dx_r.abs()
    done += _within(dx, dx_r, B_dx, "dx")
    assert dx.data_ptr() == dxv.data_ptr()
    assert _outside_untouched(dxw, lay, C) and _outside_untouched(xw, lay, C), "a byte outside the channel slice changed"
    assert torch.equal(xv.cpu(), x), "x changed"
    done += 1
    # the dead channel: every gradient exactly zero
    assert float(dg[C - 1]) == 0.0 and float(db[C - 1]) == 0.0 and bool((dx[..., C - 1] == 0).all())
    # two calls, bit for bit; and without dx the parameter gradients are the same bits
    dx2, dg2, db2 = ops.head_bn_relu_pool_bwd(xv, gpd, *dev, training)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db), "two backward calls differ"
    none, dg3, db3 = ops.head_bn_relu_pool_bwd(xv, gpd, *dev, training, need_dx=False)
    assert none is None and torch.equal(dg3, dg) and torch.equal(db3, db)
    assert _lib.last_plumbing_kernel() == R.predict(True, C, xv.data_ptr(), xv.stride(2))[0]
    return done


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_head_matches_float64(c):
    assert _run(c) == 5, "a case left out of a comparison"


def test_dense_dx_next_to_a_misaligned_x_and_the_reverse_take_the_scalar_kernel():
    """The 16-byte gate looks at BOTH views: either one off alignment, or with an odd pixel stride, is enough."""
    from kdcc_amd import _lib, ops
    c = dict(C=64, N=3, HW=35, layout="dense", training=True, shift=0.0)
    x, gamma, beta, mean, invstd, gp = _operands(c)
    dev = [t.cuda() for t in (gamma, beta, mean, invstd)]
    ref = None
    for xl, dl in (("dense", "dense"), ("slice1", "dense"), ("dense", "slice1"), ("slice4", "slice4")):
        xv, _ = _place(x, xl)
        dxv, dxw = _place(x, dl, fill=False)
        dx, dg, db = ops.head_bn_relu_pool_bwd(xv, gp.cuda(), *dev, True, out=dxv)
        assert _lib.last_plumbing_kernel() == ("head_bwd_kernel<4>" if "slice1" not in (xl, dl) else "head_bwd_kernel<1>")
        assert _outside_untouched(dxw, dl, 64)
        got = (dx.contiguous(), dg, db)
        if ref is None:
            ref = got
        if "slice1" not in (xl, dl):        # (the scalar kernel sums in another order: test_head_matches_float64 holds it to float64)
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), "the layout changed the 16-byte kernel's bits"
    odd = torch.full((3, 5, 7, 67), SENTINEL, device="cuda")           # an odd pixel stride under an aligned base
    odd[..., :64].copy_(x.cuda())
    ops.head_bn_relu_pool_fwd(odd[..., :64], *dev)
    assert _lib.last_plumbing_kernel() == "head_fwd_kernel<1>"


def test_train_mode_updates_the_running_statistics_as_bn_nhwc_apply_does():
    from kdcc_amd import ops
    c = dict(C=20, N=3, HW=35, layout="dense", training=True, shift=0.0)
    x, gamma, beta, _, _, _ = _operands(c)
    xv = x.cuda()
    g = torch.Generator().manual_seed(5)
    rm, rv = torch.randn(20, generator=g).cuda(), (torch.rand(20, generator=g) + 0.5).cuda()
    mean, invstd, var = ops.bn_nhwc_stats(xv, 1e-5)
    rm1, rv1 = rm.clone(), rv.clone()
    ops.bn_nhwc_apply(xv, gamma.cuda(), beta.cuda(), mean, invstd, var, rm1, rv1, 0.1, relu=True)
    rm2, rv2 = rm.clone(), rv.clone()
    v = rm2._version
    ops.head_bn_relu_pool_fwd(xv, gamma.cuda(), beta.cuda(), mean, invstd, var, rm2, rv2, 0.1)
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2) and not torch.equal(rm, rm2)
    assert rm2._version > v, "version-keyed caches (BN folds) must see the update"


def test_arguments_are_checked_before_anything_is_launched():
    from kdcc_amd import ops
    from kdcc_amd._lib import KdccError
    x = torch.zeros((2, 8, 8, 8), device="cuda")
    v = torch.ones(8, device="cuda")
    with pytest.raises(KdccError):
        ops.head_bn_relu_pool_fwd(x.cpu(), v, v, v, v)
    with pytest.raises(ValueError):
        ops.head_bn_relu_pool_fwd(x, v, v, v, v[:4])
    with pytest.raises(TypeError):
        ops.head_bn_relu_pool_fwd(x.bfloat16(), v, v, v, v)
    with pytest.raises(ValueError):
        ops.head_bn_relu_pool_bwd(x, torch.zeros((2, 4), device="cuda"), v, v, v, v, True)
    with pytest.raises(ValueError):
        ops.head_bn_relu_pool_bwd(x, torch.zeros((2, 8), device="cuda"), v, v, v, v, True, out=x)
