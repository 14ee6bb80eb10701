"""kd_bn_relu_maxpool2x2_fwd / _bwd (csrc/pool_ops.hip) against float64 on the CPU, evaluated on the operands as stored
(tests/_poolref.py: stock torch's max_pool2d of relu of the affine map under float64 autograd): every channel count, shape, layout
and mode of CASES, the kernel each call reached (kd_debug_last_plumbing_kernel against the restated selector), the sentinel bytes
around channel slices, two calls bit for bit, and the backward's workspace from the poisoning allocator of tests/_scratch.py.

The error bars are derived, not tuned.  With u = 2^-24 and A = |xhat gamma| + |beta| per element (A = |x| without BatchNorm), fp32
evaluation of y = (x - mean) (gamma invstd) + beta is off by at most 4 u A (a subtraction, the product gamma invstd, one fused
multiply-add, second-order slack); max is exact and 1-Lipschitz in every argument, so is relu; a sum of n terms in ANY order is off
by at most (n - 1) u sum |terms| (the recursive-summation bound) on top of the terms' own errors.  g' is the routed gradient:
gpooled at the first maximum of a window where it is positive, 0 at every other pixel; M = N H W counts every pixel:
  pooled   4 u max of A over the window
  dbeta    (M + 2) u sum |g'|                         (at most M / 4 nonzero terms, exact each; fp64 second stage)
  dgamma   (M + 4) u sum |g' xhat|                    (xhat (2 u) and the product)
  dx       |k| ((B_dbeta + |xhat| B_dgamma) / M + 8 u (|g'| + |dbeta / M| + |xhat dgamma / M|)) + 2 u |dx|  in train mode,
           4 u |dx| in eval mode and without BatchNorm  (k = gamma invstd; the tests/test_head_gpu.py bound with g' in place of
           gpooled / HW)
The routing is discontinuous, so the inputs are built such that fp32 and float64 agree on every decision (_operands asserts it):
no activation lies within 16 u A of zero, and in every window the largest positive activation exceeds every other positive one by
more than 8 u times the sum of their A -- four times the two evaluation errors -- OR the two come from bit-identical x values in the
same channel, an exact tie in both precisions.  At least one window in eight is such a deliberate tie at the maximum, the duplicate
placed at each of the four positions in turn, so the first-maximum rule decides where the gradient goes.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _poolref as R  # noqa: E402
import _scratch as S  # noqa: E402

U = 2.0 ** -24
SENTINEL = 12345.0
LAYOUTS = {"dense": (0, 0), "slice4": (4, 8), "slice1": (1, 8)}        # channel offset of the slice, extra channels of the buffer
MODES = ("train", "eval", "nobn")
SHAPES = ((2, 4, 4), (3, 5, 7), (1, 2, 2), (2, 2, 6))
CASES = [dict(C=C, N=N, H=H, W=W, layout=lay, mode=mode)
         for C, (N, H, W), lay, mode in itertools.product((1, 4, 6, 20, 64), SHAPES, LAYOUTS, MODES)]
BIG = [dict(C=64, N=8, H=32, W=32, layout="dense", mode=mode) for mode in MODES]       # 2048 windows: 42 stage-1 blocks of 48 and one of 32
assert len(CASES) == 5 * 4 * 3 * 3
ids = lambda cs: [f"C{c['C']}-N{c['N']}-{c['H']}x{c['W']}-{c['layout']}-{c['mode']}" for c in cs]
OFFS = ((0, 0), (0, 1), (1, 0), (1, 1))        # (ky, kx) in scan order


def _windows(t):
    """(N,H,W,C) -> (N,Ho,Wo,C,4): the four positions of every whole window in (ky, kx) scan order."""
    N, H, W, C = t.shape
    Ho, Wo = H // 2, W // 2
    return torch.stack([t[:, ky:2 * Ho:2, kx:2 * Wo:2, :] for ky, kx in OFFS], dim=-1)


def _stats(c, x, rm, rv):
    C = x.shape[3]
    if c["mode"] == "train":
        xd = x.double()
        return xd.mean(dim=(0, 1, 2)).float(), (1.0 / torch.sqrt(xd.var(dim=(0, 1, 2), unbiased=False) + 1e-5)).float()
    if c["mode"] == "eval":
        return rm, (1.0 / torch.sqrt(rv.double() + 1e-5)).float()
    return torch.zeros(C), torch.ones(C)


def _operands(c):
    """(x, gamma, beta, mean, invstd, gpooled, ties) fp32 on the host (gamma = beta = mean = invstd = None without BatchNorm).  With
    more than one channel the last one is dead everywhere; one gamma in three is negative; `ties` counts the windows whose maximum
    is a deliberate exact tie.  The loop ends when the post-condition of the module docstring holds, and asserts it."""
    C, N, H, W = c["C"], c["N"], c["H"], c["W"]
    bn = c["mode"] != "nobn"
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(100000 * C + 1000 * N + 10 * H + W + 7 * MODES.index(c["mode"]))
    off = torch.randn(C, generator=g) if bn else torch.zeros(C)
    x = torch.randn((N, H, W, C), generator=g) * 1.5 + off
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1                                  # (a negative gamma flips which side of the mean is active)
    beta = torch.randn(C, generator=g) * 0.3
    dead = C > 1
    if not bn:
        gamma, beta = torch.ones(C), torch.zeros(C)
        if dead:
            x[..., C - 1] = -x[..., C - 1].abs() - 1.0
    elif dead:
        beta[C - 1] = -60.0                           # |xhat gamma| stays far below: the channel is dead everywhere
    gp = torch.randn((N, Ho, Wo, C), generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    # the deliberate ties: every fourth (window, channel) pair in a fixed walk; the pair's two positions cycle through all twelve
    # ordered choices, so the duplicate of the maximum lands at each of the four positions, before and behind the original
    live = C - 1 if dead else C
    pairs = [(p, q) for p in range(4) for q in range(4) if p != q]
    sgn = torch.sign(gamma)
    n_tie = 0
    for i, (n, ho, wo, ch) in enumerate(itertools.product(range(N), range(Ho), range(Wo), range(live))):
        if i % 4:
            continue
        (py, px), (qy, qx) = (OFFS[k] for k in pairs[n_tie % 12])
        v = off[ch] + sgn[ch] * (6.0 + 0.37 * (n_tie % 5))          # four sigma on the active side: the window's maximum
        x[n, 2 * ho + py, 2 * wo + px, ch] = v
        x[n, 2 * ho + qy, 2 * wo + qx, ch] = v
        n_tie += 1
    for _ in range(24):
        mean, invstd = _stats(c, x, rm, rv)
        xhat = (x.double() - mean.double()) * invstd.double()
        y = xhat * gamma.double() + beta.double()
        A = (xhat * gamma.double()).abs() + beta.double().abs()
        close = y.abs() <= 16 * U * A
        yw, Aw, xw = _windows(y), _windows(A), _windows(x)
        top = yw.argmax(dim=-1, keepdim=True)
        yt, At, xt = yw.gather(-1, top), Aw.gather(-1, top), xw.gather(-1, top)
        other = torch.ones_like(yw, dtype=torch.bool).scatter_(-1, top, False)
        near = other & (yt > 0) & (yw > 0) & (yt - yw <= 8 * U * (At + Aw)) & (xw != xt)
        if not bool(close.any()) and not bool(near.any()):
            break
        x = torch.where(close, x + 0.25, x)
        # a runner-up too near the maximum moves a quarter towards the inactive side (written back through the window views)
        step = (0.25 * sgn).view(1, 1, 1, C)
        for k, (ky, kx) in enumerate(OFFS):
            v = x[:, ky:2 * Ho:2, kx:2 * Wo:2, :]
            v.copy_(torch.where(near[..., k], v - step, v))
    assert not bool(close.any()), "an activation too close to zero for its sign to be certain in fp32"
    assert not bool(near.any()), "two activations of a window too close for their order to be certain in fp32"
    if dead:
        assert bool((y[..., C - 1] < -0.5).all())
    tied = ((xw == xt) & other & (yt > 0)).any(dim=-1)
    ties = int(tied.sum())
    if not bn:
        gamma = beta = mean = invstd = None
    return x, gamma, beta, mean, invstd, gp, ties


def test_the_construction_ties_one_window_in_eight_at_every_position():
    """(No kernel runs here.)  Over the cases, deliberate ties make up at least an eighth of the windows of the live channels, and the
    float64 routing sends a tied window's gradient to the FIRST of the tied positions, each of the four positions being that first one
    somewhere and the skipped duplicate somewhere."""
    first, skipped = set(), set()
    for c in CASES[::4] + BIG[:1]:
        x, gamma, beta, mean, invstd, gp, ties = _operands(c)
        live = c["C"] - 1 if c["C"] > 1 else 1
        assert 8 * ties >= c["N"] * (c["H"] // 2) * (c["W"] // 2) * live, c
        _, _, _, _, y, gq = R.pool_ref(x, gamma, beta, mean, invstd, torch.ones_like(gp), c["mode"] == "train")
        yw, gw = _windows(y), _windows(gq)
        tie = (yw == yw.max(dim=-1, keepdim=True).values) & (yw > 0)
        for k in range(4):
            first |= {k} if bool((tie[..., k] & (gw[..., k] == 1) & (tie.sum(-1) > 1)).any()) else set()
            skipped |= {k} if bool((tie[..., k] & (gw[..., k] == 0)).any()) else set()
        assert bool((gw.sum(-1) <= 1).all()) and not bool((tie[..., 1:] & (gw[..., 1:] == 1) & tie[..., :1]).any())
    assert first == {0, 1, 2} and skipped == {1, 2, 3}


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


def _views(*ts):
    return tuple((t.data_ptr(), t.stride(2)) if t is not None else (0, 0) for t in ts)


def _run(c, monkeypatch=None):
    """Both entry points on one case; returns the number of comparisons made."""
    from kdcc_amd import _lib, ops
    C, N, H, W, lay, mode = c["C"], c["N"], c["H"], c["W"], c["layout"], c["mode"]
    bn, training = mode != "nobn", mode == "train"
    M = N * H * W
    x, gamma, beta, mean, invstd, gp, _ = _operands(c)
    p_r, dx_r, dg_r, db_r, y, gq = R.pool_ref(x, gamma, beta, mean, invstd, gp, training)
    if bn:
        xhat = (x.double() - mean.double()) * invstd.double()
        A = (xhat * gamma.double()).abs() + beta.double().abs()
    else:
        xhat, A = x.double(), x.double().abs()
    xv, xw = _place(x, lay)
    dev = [t.cuda() for t in (gamma, beta, mean, invstd)] if bn else []
    done = 0
    # ---- forward, y into a view of the same layout
    yv, yw = _place(p_r, lay, fill=False)
    pooled = ops.bn_relu_maxpool2x2_fwd(xv, *dev, out=yv)
    want = R.predict(False, bn, N, H, W, C, _views(xv, yv))
    assert _lib.last_plumbing_kernel() == want["name"] and (want["vec"] == 4) == (lay != "slice1" and C % 4 == 0)
    done += _within(pooled, p_r, 4 * U * _windows(A).max(dim=-1).values, "pooled")
    assert pooled.data_ptr() == yv.data_ptr() and _outside_untouched(yw, lay, C), "a byte outside the channel slice of y changed"
    assert torch.equal(pooled, ops.bn_relu_maxpool2x2_fwd(xv, *dev)), "two forward calls differ"
    if C > 1:
        assert bool((pooled[..., C - 1] == 0).all())
    # ---- backward, gpooled and dx in views of the same layout
    gv, _ = _place(gp, lay)
    dxv, dxw = _place(x, lay, fill=False)
    call = lambda **kw: ops.bn_relu_maxpool2x2_bwd(xv, gv, *dev, training=training, **kw)
    if monkeypatch is None:
        dx, dg, db = call(out=dxv)
    else:                   # the workspace from the poisoning allocator: the same bits whatever it held, and no byte past its end
        outs = []
        for fill in S.FILLS:
            with S.poison(monkeypatch, ops, fill, key=f"pool:{mode}") as p:
                outs.append(call(out=dxv))
                outs[-1] = tuple(None if t is None else t.clone() for t in outs[-1])
            assert p.count == (1 if bn else 0), "one workspace for the BatchNorm form, none without"
            for b in p.buffers:
                assert b.entry == "bn_relu_maxpool2x2_bwd" and b.high_water() <= R.predict(True, True, N, H, W, C, _views(xv, gv, dxv))["ws"]
        for o in outs[1:]:
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(o, outs[0])), "the result depends on what the scratch held"
        dx, dg, db = call(out=dxv)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip((dx, dg, db), outs[0]))
    want = R.predict(True, bn, N, H, W, C, _views(xv, gv, dxv))
    assert _lib.last_plumbing_kernel() == want["name"] and (want["vec"] == 4) == (lay != "slice1" and C % 4 == 0)
    if bn:
        B_db = (M + 2) * U * gq.abs().sum(dim=(0, 1, 2))
        B_dg = (M + 4) * U * (gq * xhat).abs().sum(dim=(0, 1, 2))
        done += _within(db, db_r, B_db, "dbeta")
        done += _within(dg, dg_r, B_dg, "dgamma")
        k = (gamma.double() * invstd.double()).abs()
    else:
        assert dg is None and db is None
        done += 2
    if training:
        B_dx = k * ((B_db + xhat.abs() * B_dg) / M + 8 * U * (gq.abs() + (db_r / M).abs() + (xhat * dg_r / M).abs())) + 2 * U * dx_r.abs()
    else:
        B_dx = 4 * U * dx_r.abs()
    done += _within(dx, dx_r, B_dx, "dx")
    assert dx.data_ptr() == dxv.data_ptr()
    assert _outside_untouched(dxw, lay, C) and _outside_untouched(xw, lay, C), "a byte outside the channel slice changed"
    assert torch.equal(xv.cpu(), x), "x changed"
    done += 1
    # where no gradient is routed -- non-maximal pixels, a dropped odd row or column -- train mode still writes the mean terms
    unrouted = gq == 0
    if C > 1:
        unrouted[..., C - 1] = False
    if training:
        sure = unrouted & (dx_r.abs() > 2 * B_dx)
        assert bool(sure.any()) and bool((dx.cpu()[sure] != 0).all()), "the mean terms are missing where no gradient is routed"
        if H % 2:
            assert bool(sure[:, H - 1].any()), "the dropped row has mean terms"
        if W % 2:
            assert bool(sure[:, :, W - 1].any()), "the dropped column has mean terms"
    else:
        assert bool((dx.cpu()[unrouted] == 0).all())
    # the dead channel: every gradient exactly zero
    if C > 1:
        assert bool((dx[..., C - 1] == 0).all()) and (not bn or (float(dg[C - 1]) == 0.0 and float(db[C - 1]) == 0.0))
    # two calls, bit for bit; and without dx the parameter gradients are the same bits
    dx2, dg2, db2 = call()
    assert torch.equal(dx2, dx) and (not bn or (torch.equal(dg2, dg) and torch.equal(db2, db))), "two backward calls differ"
    if bn:
        none, dg3, db3 = call(need_dx=False)
        assert none is None and torch.equal(dg3, dg) and torch.equal(db3, db)
        assert _lib.last_plumbing_kernel() == R.predict(True, True, N, H, W, C, _views(xv, gv, None))["name"]
    return done


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_pool_matches_float64(c):
    assert _run(c) == 5, "a case left out of a comparison"


@pytest.mark.parametrize("c", BIG, ids=ids(BIG))
def test_several_stage1_blocks_with_a_ragged_last_one_on_poisoned_scratch(c, monkeypatch):
    want = R.predict(True, True, c["N"], c["H"], c["W"], c["C"], ((0, 0),))
    assert want["nwb"] > 2 and want["windows"] % R.WINS, "several window blocks, the last one short"
    assert _run(c, monkeypatch) == 5


def test_any_view_off_alignment_takes_the_scalar_kernels():
    """The 16-byte gate looks at EVERY view of the call: one off alignment, or with an odd pixel stride, is enough."""
    from kdcc_amd import _lib, ops
    c = dict(C=64, N=3, H=5, W=7, layout="dense", mode="train")
    x, gamma, beta, mean, invstd, gp, _ = _operands(c)
    dev = [t.cuda() for t in (gamma, beta, mean, invstd)]
    ref = None
    for xl, gl, dl in (("dense",) * 3, ("slice1", "dense", "dense"), ("dense", "slice1", "dense"), ("dense", "dense", "slice1"), ("slice4",) * 3):
        xv, _ = _place(x, xl)
        gv, _ = _place(gp, gl)
        dxv, dxw = _place(x, dl, fill=False)
        dx, dg, db = ops.bn_relu_maxpool2x2_bwd(xv, gv, *dev, training=True, out=dxv)
        scalar = "slice1" in (xl, gl, dl)
        assert _lib.last_plumbing_kernel() == ("pool_bwd_kernel<1>" if scalar else "pool_bwd_kernel<4>")
        assert _outside_untouched(dxw, dl, 64)
        yv, yw = _place(gp, gl, fill=False)
        ops.bn_relu_maxpool2x2_fwd(xv, *dev, out=yv)
        assert _lib.last_plumbing_kernel() == ("pool_fwd_kernel<1>" if "slice1" in (xl, gl) else "pool_fwd_kernel<4>")
        assert _outside_untouched(yw, gl, 64)
        got = (dx.contiguous(), dg, db, yv.contiguous())
        if ref is None:
            ref = got
        assert torch.equal(got[3], ref[3]), "the forward is elementwise: the same bits at either width"
        if not scalar:      # (the scalar kernel sums in another order: test_pool_matches_float64 holds it to float64)
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), "the layout changed the 16-byte kernel's bits"
    odd = torch.full((3, 5, 7, 67), SENTINEL, device="cuda")           # an odd pixel stride under an aligned base
    odd[..., :64].copy_(x.cuda())
    ops.bn_relu_maxpool2x2_fwd(odd[..., :64], *dev)
    assert _lib.last_plumbing_kernel() == "pool_fwd_kernel<1>"


def test_train_mode_updates_the_running_statistics_as_bn_nhwc_apply_does():
    from kdcc_amd import ops
    c = dict(C=20, N=3, H=5, W=7, layout="dense", mode="train")
    x, gamma, beta, _, _, _, _ = _operands(c)
    xv = x.cuda()
    g = torch.Generator().manual_seed(5)
    rm, rv = torch.randn(20, generator=g).cuda(), (torch.rand(20, generator=g) + 0.5).cuda()
    mean, invstd, var = ops.bn_nhwc_stats(xv, 1e-5)
    rm1, rv1 = rm.clone(), rv.clone()
    ops.bn_nhwc_apply(xv, gamma.cuda(), beta.cuda(), mean, invstd, var, rm1, rv1, 0.1, relu=True)
    rm2, rv2 = rm.clone(), rv.clone()
    v = rm2._version
    ops.bn_relu_maxpool2x2_fwd(xv, gamma.cuda(), beta.cuda(), mean, invstd, var, rm2, rv2, 0.1)
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2) and not torch.equal(rm, rm2)
    assert rm2._version > v, "version-keyed caches (BN folds) must see the update"


def test_a_map_without_a_window_is_refused_before_anything_is_launched():
    from kdcc_amd import _lib, ops
    from kdcc_amd._lib import KdccError
    KD_ERR_INVALID = -1                 # include/kdcc.h
    v = torch.ones(8, device="cuda")
    ok = torch.zeros((2, 2, 2, 8), device="cuda")
    ops.bn_relu_maxpool2x2_bwd(ok, torch.zeros((2, 1, 1, 8), device="cuda"), v, v, v, v, training=True)
    assert _lib.last_plumbing_kernel().startswith("pool_bwd_kernel")
    for shape in ((2, 1, 4, 8), (2, 4, 1, 8)):
        x = torch.zeros(shape, device="cuda")
        with pytest.raises(KdccError, match=f"rc={KD_ERR_INVALID}"):
            ops.bn_relu_maxpool2x2_fwd(x, v, v, v, v)
        y = torch.full((2, 1, 1, 8), SENTINEL, device="cuda")
        rc = _lib.lib().kd_bn_relu_maxpool2x2_fwd(x.data_ptr(), 8, *shape, v.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), y.data_ptr(), 8,
                                                 None, None, None, 0.0, None)
        torch.cuda.synchronize()
        assert rc == KD_ERR_INVALID and bool((y == SENTINEL).all())
        assert _lib.last_plumbing_kernel().startswith("pool_bwd_kernel"), "the refused call noted (and launched) nothing"
    with pytest.raises(KdccError):
        ops.bn_relu_maxpool2x2_fwd(ok.cpu(), v, v, v, v)
    with pytest.raises(ValueError):
        ops.bn_relu_maxpool2x2_fwd(ok, v, v, v, v[:4])
    with pytest.raises(ValueError):
        ops.bn_relu_maxpool2x2_fwd(ok, v, v, None, None)
    with pytest.raises(TypeError):
        ops.bn_relu_maxpool2x2_fwd(ok.bfloat16(), v, v, v, v)
    with pytest.raises(ValueError):
        ops.bn_relu_maxpool2x2_bwd(ok, torch.zeros((2, 2, 2, 8), device="cuda"), v, v, v, v, training=True)
    with pytest.raises(ValueError):
        ops.bn_relu_maxpool2x2_bwd(ok, torch.zeros((2, 1, 1, 8), device="cuda"), v, v, v, v, training=True, out=ok)
