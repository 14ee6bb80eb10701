"""Every dispatch branch of the criterion, metric and optimizer entry points of csrc/losses.hip against float64 on the CPU,
evaluated on the inputs as stored (tests/_loss_dispatch_cases.py).

Each row asserts the kernel it reached (kd_debug_last_plumbing_kernel).  Bars: integer and 0 / 1 results (confusion matrices, the
top-k mask) are exact; elementwise results use test_ops_gpu.assert_close for the storage dtype; scalar losses rtol = 1e-4, the bar
test_criteria_gpu._bar holds these entry points to; the reduction rows that bite use the recursive-summation bound with the chain
length of the kernel's own decomposition.  A row marked ill-conditioned takes max(that bar, 3 x the deviation of the same
reference formula evaluated in fp32 on the CPU), the goldens' rule; never anything derived from the kernel's output.  Every row
that returns a gradient runs twice and must repeat bit for bit (fixed-order reductions).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _loss_dispatch_cases as L
from test_ops_gpu import assert_close

pytestmark = pytest.mark.gpu

DT = L.DT


@pytest.fixture(scope="module")
def K():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    assert torch.cuda.is_available()
    return ops


def lib():
    from kdcc_amd import _lib
    return _lib


def note():
    return lib().last_plumbing_kernel()


def reached(c):
    got = note()
    print(f"{c['id']}: reached {got}")
    assert got == c["kernel"], f"{c['id']}: dispatched to {got}, this row is meant to cover {c['kernel']}"


# ------------------------------------------------------------------------------------------------------ operands and their buffers
def carve(shape, lay, make):
    """(logical view, whole buffer) of an operand in layout `lay`; make(shape) allocates."""
    if len(shape) == 2:
        N, Cc = shape
        if lay == "2d":
            buf = make((N, Cc))
            return buf, buf
        buf = make((N, Cc + 16))
        return buf[:, 8:8 + Cc], buf
    N, Cc, H, W = shape
    if lay == "nchw":
        buf = make((N, Cc, H, W))
        return buf, buf
    if lay == "cl":
        buf = make((N, H, W, Cc))
        return buf.permute(0, 3, 1, 2), buf
    if lay == "cs":
        buf = make((N, H, W, Cc + 16))
        return buf[..., 8:8 + Cc].permute(0, 3, 1, 2), buf
    if lay == "bs":
        buf = make((N, H + 1, W, Cc))
        return buf[:, :H].permute(0, 3, 1, 2), buf
    assert lay == "off1"
    buf = make((N * H * W * Cc + 1,))
    return buf[1:].view(N, H, W, Cc).permute(0, 3, 1, 2), buf


def blank(shape, dt, lay, K=None):
    """(view, buffer) filled with the sentinel."""
    v, b = carve(tuple(shape), lay, lambda s: torch.full(s, L.SENTINEL, dtype=DT[dt], device="cuda"))
    if K is not None:
        vv, (N, Cc, P) = K.view3(v)
        assert (vv.sN, vv.sC, vv.sP) == L.strides(lay, tuple(shape)), f"the table's strides of {lay} are not the device tensor's"
        assert (v.data_ptr() % 16 == 0) == L.aligned16(lay, dt)
    return v, b


def dev(a, dt, lay, K=None):
    v, b = blank(a.shape, dt, lay, K)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DT[dt]))
    return v, b


def untouched(shape, lay, buf, what=""):
    """Everything of `buf` outside the operand's view still holds the sentinel."""
    mv, mb = carve(tuple(shape), lay, lambda s: torch.ones(s, dtype=torch.bool, device="cuda"))
    mv[...] = False
    assert bool((buf[mb].float() == L.SENTINEL).all()), f"{what}: wrote outside the view"


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scalar_ok(got, ref, bound, what):
    err = abs(float(got) - ref)
    print(f"{what}: got {float(got)!r} ref {ref!r} err/bound {err / max(bound, 1e-300):.3e}")
    assert err <= bound, f"{what}: |{float(got)!r} - {ref!r}| = {err:.3e} > {bound:.3e}"


def grad_ok(got, ref, dt, what, ref32=None):
    """test_ops_gpu.assert_close; with ref32 (the reference formula evaluated in fp32) each of its two bars becomes
    max(bar, 3 x the fp32 evaluation's own deviation)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-6)
    den = max((ref ** 2).sum(), 1e-30)
    err, l2 = np.abs(got - ref).max() / scale, np.sqrt(((got - ref) ** 2).sum() / den)
    tol, tol2 = (1e-3, 2e-4) if dt == "f32" else (1.5e-2, 5e-3)
    if ref32 is None:
        print(f"{what}: max err / range {err:.3e} (bar {tol:g}), relative L2 {l2:.3e} (bar {tol2:g})")
        assert_close(got, ref, dt, what)
        return
    d_err, d_l2 = np.abs(ref32 - ref).max() / scale, np.sqrt(((ref32 - ref) ** 2).sum() / den)
    print(f"{what}: max err / range {err:.3e} (bar {tol:g}, fp32 evaluation {d_err:.3e}), relative L2 {l2:.3e} (bar {tol2:g}, fp32 evaluation {d_l2:.3e})")
    assert err <= max(tol, 3 * d_err) and l2 <= max(tol2, 3 * d_l2), what


def same_bits(a, b, what):
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{what}: two runs differ"


def set_note(K):
    """Leaves a known note behind, so that a refused call can be seen to have launched nothing."""
    K.scale_by_device_scalar_(torch.ones(8, device="cuda"), torch.ones(1, device="cuda"))
    assert note() == "scale_by_device_scalar_kernel<f32>"
    return note()


# --------------------------------------------------------------------------- the two-operand entry points through their C interface
def two_operand_call(K, fn, s, t, extra, grad, grad_scale=1.0):
    """What ops._pair_loss does, with a gradient view of the caller's (a slice, another storage type)."""
    vs, (N, Cc, P) = K.view3(s)
    vt, _ = K.view3(t)
    vg = K.view3(grad)[0] if grad is not None else None
    loss = torch.empty((), dtype=torch.float32, device="cuda")
    ws, need = K.loss_workspace(N, Cc, P, s.device)
    own = [K._ptr(e) if torch.is_tensor(e) else e for e in extra]
    lib().check(getattr(lib().lib(), fn)(C.byref(vs), C.byref(vt), *own, N, Cc, P, K._ptr(loss), C.byref(vg) if vg is not None else None,
                                         C.c_float(grad_scale), K._ptr(ws), need, K.stream_ptr()), fn)
    return loss


def run_two_operand(K, c, fn, wrapper, extra, inp):
    """-> (loss, grad or None) of one call; the wrapper when it allocates the gradient the row asks for, the C interface otherwise."""
    ls, lt, lg = L.lays(c)
    s, _ = dev(inp["s"], c["sdt"], ls, K)
    t, _ = dev(inp["t"], c["tdt"], lt, K)
    gdt = c.get("gdt")
    if lg is None or (lg == ls and ls in ("cl", "nchw", "2d") and gdt == c["sdt"]):
        loss, grad = wrapper(s, t, lg is not None, extra)
        if grad is not None:
            assert K.view3(grad)[0].sC == K.view3(s)[0].sC
        return loss, grad
    grad, gbuf = blank(c["shape"], gdt, lg, K)
    loss = two_operand_call(K, fn, s, t, extra, grad)
    untouched(c["shape"], lg, gbuf, c["id"])
    return loss, grad


def check_two_operand(K, c, fn, wrapper, extra_of):
    inp, ref = L.build(c)
    extra = extra_of(inp)
    loss, grad = run_two_operand(K, c, fn, wrapper, extra, inp)
    reached(c)
    bound = L.loss_bound(c, ref)
    if c.get("illcond"):
        dev32 = abs(ref["loss32"] - ref["loss"])
        print(f"{c['id']}: loss bar {bound:.3e}, fp32 evaluation off by {dev32:.3e}")
        bound = max(bound, 3 * dev32)
    scalar_ok(loss, ref["loss"], bound, f"{c['id']} loss")
    if grad is not None:
        grad_ok(host(grad), ref["grad"], c["gdt"], f"{c['id']} grad", ref.get("grad32"))
        loss2, grad2 = run_two_operand(K, c, fn, wrapper, extra, inp)
        same_bits(loss.reshape(1), loss2.reshape(1), f"{c['id']} loss")
        same_bits(grad, grad2, f"{c['id']} grad")
    return inp, ref, loss, grad


PAIR = L.cases_of("pair")
PAIR_FN = {"kld": "kd_kldiv", "jsd": "kd_jsdiv", "ekl": "kd_ensemble_kldiv"}


@pytest.mark.parametrize("c", PAIR, ids=L.ids(PAIR))
def test_pair(K, c):
    T = c["T"]
    wrapper = {"kld": lambda s, t, want_grad, extra: K.kldiv(s, t, T, want_grad=want_grad),
               "jsd": lambda s, t, want_grad, extra: K.jsdiv(s, t, T, want_grad=want_grad),
               "ekl": lambda s, t, want_grad, extra: K.ensemble_kldiv(s, t, want_grad=want_grad)}[c["kind"]]
    check_two_operand(K, c, PAIR_FN[c["kind"]], wrapper, lambda inp: () if c["kind"] == "ekl" else (C.c_float(T),))


MSE = L.cases_of("hint_mse")


@pytest.mark.parametrize("c", MSE, ids=L.ids(MSE))
def test_hint_mse(K, c):
    check_two_operand(K, c, "kd_hint_mse", lambda s, t, want_grad, extra: K.hint_mse(s, t, 19.0, want_grad=want_grad), lambda inp: (C.c_float(inp["num_classes"]),))


WH = L.cases_of("whmse")


@pytest.mark.parametrize("c", WH, ids=L.ids(WH))
def test_weighted_hint_mse(K, c):
    check_two_operand(K, c, "kd_weighted_hint_mse", lambda s, t, want_grad, extra: K.weighted_hint_mse(s, t, extra[0], want_grad=want_grad),
                      lambda inp: (cu(inp["w"]), int(c["per_sample"])))


TK = L.cases_of("topk")


def topk_call(K, c, inp):
    """-> (loss, grad or None, mask); through the C interface (a K the wrapper would refuse itself, a sliced gradient)."""
    ls, lt, lg = L.lays(c)
    s, _ = dev(inp["s"], c["sdt"], ls, K)
    t, _ = dev(inp["t"], c["tdt"], lt, K)
    if not c.get("refused") and (lg is None or (lg == ls and ls in ("cl", "nchw"))):
        return K.topk_hint_mse(s, t, c["k"], want_grad=lg is not None, want_mask=True)
    vs, (N, Cc, P) = K.view3(s)
    vt, _ = K.view3(t)
    grad, gbuf = blank(c["shape"], c["gdt"], lg, K)
    vg = K.view3(grad)[0]
    loss = torch.empty((), dtype=torch.float32, device="cuda")
    mask = torch.empty((N, Cc), dtype=torch.float32, device="cuda")
    need = lib().lib().kd_topk_hint_workspace(N, Cc, P)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    lib().check(lib().lib().kd_topk_hint_mse(C.byref(vs), C.byref(vt), c["k"], N, Cc, P, K._ptr(loss), C.byref(vg), C.c_float(1.0), K._ptr(mask),
                                             K._ptr(ws), need, K.stream_ptr()), "kd_topk_hint_mse")
    untouched(c["shape"], lg, gbuf, c["id"])
    return loss, grad, mask


@pytest.mark.parametrize("c", TK, ids=L.ids(TK))
def test_topk_hint_mse(K, c):
    inp, ref = L.build(c)
    if c.get("refused"):
        before = set_note(K)
        with pytest.raises(lib().KdccError):
            topk_call(K, c, inp)
        assert note() == before, "a refused call noted a kernel"
        return
    loss, grad, mask = topk_call(K, c, inp)
    reached(c)
    assert np.array_equal(host(mask), ref["mask"]), f"{c['id']}: mask"
    if c.get("tie"):
        for n, (lo, hi) in enumerate(inp["tie"]):
            assert host(mask)[n, lo] == 1.0 and host(mask)[n, hi] == 0.0, "equal norms: the lower channel is kept"
    scalar_ok(loss, ref["loss"], L.loss_bound(c, ref), f"{c['id']} loss")
    if grad is not None:
        grad_ok(host(grad), ref["grad"], c["gdt"], f"{c['id']} grad")
        loss2, grad2, mask2 = topk_call(K, c, inp)
        same_bits(loss.reshape(1), loss2.reshape(1), c["id"])
        same_bits(grad, grad2, c["id"])


# ------------------------------------------------------------------------------------------------------------- cross entropy
CE = L.cases_of("ce2d")


@pytest.mark.parametrize("c", CE, ids=L.ids(CE))
def test_ce2d(K, c):
    inp, ref = L.build(c)
    x, _ = dev(inp["x"], c["dt"], c["lay"], K)
    loss = K.ce2d(x, cu(inp["y"]), 255, cu(inp["w"]), c.get("size_average", True))
    reached(c)
    scalar_ok(loss, ref["loss"], L.loss_bound(c, ref), f"{c['id']} loss")


CEG = L.cases_of("ce2d_grad")


def ce_grad_call(K, c, inp):
    x, _ = dev(inp["x"], c["dt"], c["lay"], K)
    y, w, sa = cu(inp["y"]), cu(inp["w"]), c.get("size_average", True)
    if c["lay"] in ("cl", "nchw"):
        return K.ce2d_grad(x, y, 255, 1.0, w, sa)
    grad, gbuf = blank(c["shape"], c["dt"], c["lay"], K)
    vx, (N, Cc, P) = K.view3(x)
    vg, _ = K.view3(grad)
    ws, need = K.loss_workspace(N, Cc, P, x.device)
    lib().check(lib().lib().kd_ce2d_weighted_grad(C.byref(vx), K._ptr(y), K._ptr(w), int(not sa), 255, N, Cc, P, C.byref(vg), C.c_float(1.0),
                                                  K._ptr(ws), need, K.stream_ptr()), "kd_ce2d_weighted_grad")
    untouched(c["shape"], c["lay"], gbuf, c["id"])
    return grad


@pytest.mark.parametrize("c", CEG, ids=L.ids(CEG))
def test_ce2d_grad(K, c):
    inp, ref = L.build(c)
    grad = ce_grad_call(K, c, inp)
    reached(c)
    grad_ok(host(grad), ref["grad"], c["dt"], f"{c['id']} grad")
    if c.get("all_ignored"):
        assert not host(grad).any(), "every pixel ignored: the gradient is 0, not NaN"
    same_bits(grad, ce_grad_call(K, c, inp), c["id"])


CF = L.cases_of("confusion")


@pytest.mark.parametrize("c", CF, ids=L.ids(CF))
def test_confusion(K, c):
    inp, ref = L.build(c)
    x, _ = dev(inp["x"], c["dt"], c["lay"], K)
    conf = K.confusion(x, cu(inp["y"]), cu(inp["conf0"]) if c.get("accumulate") else None, bool(c.get("accumulate")))
    reached(c)
    got = conf.cpu().numpy()
    print(f"{c['id']}: {int(np.abs(got - ref['conf']).sum())} counts differ of {int(ref['conf'].sum())}")
    assert np.array_equal(got, ref["conf"])


# ------------------------------------------------------------------------------------------------ from the low-resolution logits
UPS = L.cases_of("ce2d_up", "kldiv_up", "jsdiv_up", "focal_up", "metrics_up")


def up_call(K, c, inp, reduction="mean"):
    N, h, w, Cc, H, W = c["geom"]
    s, t, y = cu(inp["s"]), cu(inp["t"]), cu(inp["y"])
    op = c["op"]
    if op == "ce2d_up":
        return K.ce2d_up(s, y, (H, W), 255, c["ac"])
    if op == "kldiv_up":
        return K.kldiv_up(s, t, (H, W), 2.0, c["ac"])
    if op == "jsdiv_up":
        return K.jsdiv_up(s, t, (H, W), 2.0, c["ac"])
    if op == "focal_up":
        return K.focal_up(s, y, (H, W), 2.0, cu(inp.get("alpha", np.ones(Cc, np.float32))), -100, reduction, c["ac"])
    return K.logit_metrics_up(s, t, y, (H, W), 255, c["ac"])


@pytest.mark.parametrize("c", UPS, ids=L.ids(UPS))
def test_up(K, c):
    inp, ref = L.build(c)
    if c.get("refused"):
        before = set_note(K)
        with pytest.raises(lib().KdccError):
            up_call(K, c, inp)
        assert note() == before, "a refused call noted a kernel"
        return
    op = c["op"]
    out = up_call(K, c, inp)
    reached(c)
    if op == "focal_up":
        for red in ("mean", "sum"):
            loss, stats = up_call(K, c, inp, red)
            scalar_ok(loss, ref[red], 1e-4 * abs(ref[red]), f"{c['id']} {red}")
            for i, nm in enumerate(("sum a", "sum ce", "sum w")):
                scalar_ok(stats[i], ref["stats"][i], 1e-4 * abs(ref["stats"][i]), f"{c['id']} {nm}")
    elif op == "metrics_up":
        vals, conf_s, conf_t = out
        for i, nm in enumerate(("ce(s)", "ce(t)", "mse")):
            scalar_ok(vals[i], ref["out"][i], 1e-4 * abs(ref["out"][i]), f"{c['id']} {nm}")
        print(f"{c['id']}: {inp['near_ties']} pixels carry the label 255 ({int(ref['conf_s'].sum())} counted)")
        assert np.array_equal(conf_s.cpu().numpy(), ref["conf_s"]), f"{c['id']} conf_s"
        assert np.array_equal(conf_t.cpu().numpy(), ref["conf_t"]), f"{c['id']} conf_t"
    else:
        scalar_ok(out, ref["loss"], L.loss_bound(c, ref), f"{c['id']} loss")


# --------------------------------------------------------------------------------------------------------------------- focal
FO = L.cases_of("focal", "focal_grad")


def focal_call(K, c, inp):
    x, _ = dev(inp["x"], c["dt"], c["lay"], K)
    y, alpha = cu(inp["y"]), cu(inp["alpha"])
    loss, stats, amap, cemap = K.focal(x, y, c["gamma"], alpha, -100, c["red"], want_maps=c.get("maps", True))
    assert (amap is not None) == c.get("maps", True)
    fwd_note = note()
    grad = None
    if c["op"] == "focal_grad":
        grad = K.focal_grad(x, y, c["gamma"], alpha, -100, c["red"], cu(inp["up"]), stats, amap, cemap)
    return fwd_note, loss, stats, amap, cemap, grad


@pytest.mark.parametrize("c", FO, ids=L.ids(FO))
def test_focal(K, c):
    inp, ref = L.build(c)
    fwd_note, loss, stats, amap, cemap, grad = focal_call(K, c, inp)
    assert fwd_note == "focal_kernel"
    reached(c)
    if c["op"] == "focal":
        if c["red"] != "none":
            scalar_ok(loss, ref["loss"], 1e-4 * abs(ref["loss"]), f"{c['id']} loss")
        for i, nm in enumerate(("sum a", "sum ce", "sum w")):
            scalar_ok(stats[i], ref["stats"][i], 1e-4 * abs(ref["stats"][i]), f"{c['id']} {nm}")
        if c.get("maps", True):
            grad_ok(host(amap), ref["a_map"], "f32", f"{c['id']} a_map")
            grad_ok(host(cemap), ref["ce_map"], "f32", f"{c['id']} ce_map")
    else:
        grad_ok(host(grad), ref["grad"], c["dt"], f"{c['id']} grad")
        same_bits(grad, focal_call(K, c, inp)[5], c["id"])


# ----------------------------------------------------------------------------------------------- the ensemble's criterion and mean
MT = L.cases_of("kldiv_multi", "softmax_mean")


def multi_call(K, c, inp):
    s, _ = dev(inp["s"], c["dt"], c["lay"], K)
    ts = [dev(t, c["dt"], c["lay"])[0] for t in inp["ts"]]
    ts, w = (ts * 17)[:c["nt"]], (inp["w"] * 17)[:c["nt"]]
    if c["op"] == "softmax_mean":
        return K.softmax_mean(ts, w, inp["T"])
    return K.kldiv_multi(s, ts, w, inp["T"], cu(inp["y"]), 255, inp["kd_scale"], inp["sup_scale"], want_grad=c.get("grad", True))


@pytest.mark.parametrize("c", MT, ids=L.ids(MT))
def test_kldiv_multi_and_softmax_mean(K, c):
    inp, ref = L.build(c)
    if c.get("refused"):
        before = set_note(K)
        with pytest.raises(lib().KdccError):
            multi_call(K, c, inp)
        assert note() == before, "a refused call noted a kernel"
        return
    out = multi_call(K, c, inp)
    reached(c)
    if c["op"] == "softmax_mean":
        assert out.dtype == torch.float32
        grad_ok(host(out), ref["out"], "f32", f"{c['id']} out")
        return
    kd, sup, total, grad = out
    for nm, v in (("kd", kd), ("sup", sup), ("total", total)):
        scalar_ok(v, ref[nm], 1e-4 * abs(ref[nm]), f"{c['id']} {nm}")
    if c.get("grad", True):
        grad_ok(host(grad), ref["grad"], c["dt"], f"{c['id']} grad")
        out2 = multi_call(K, c, inp)
        same_bits(torch.stack([kd, sup, total]), torch.stack(list(out2[:3])), c["id"])
        same_bits(grad, out2[3], c["id"])
    else:
        assert grad is None


# --------------------------------------------------------------------------------------------------------------------- RAdam
RA = L.cases_of("radam", "radam_multi")


@pytest.mark.parametrize("c", RA, ids=L.ids(RA))
def test_radam(K, c):
    inp, ref = L.build(c)
    hp = L.RADAM_HP
    items = []
    for t in inp["tensors"]:
        p, g, m, v = (cu(t[k]) for k in "pgmv")
        items.append((p, g, m, v, t["step"], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], t["wd"]))
    if c["op"] == "radam":
        K.radam_step(*items[0])
    else:
        K.radam_step_multi(items)
    reached(c)
    for i, (t, (rp, rm, rv), it) in enumerate(zip(inp["tensors"], ref["tensors"], items)):
        what = f"{c['id']} tensor {i} (step {t['step']}, weight decay {t['wd']:g}, {t['p'].size} elements)"
        # the update, not the parameter: a weight decay of lr * wd = 1e-3 of p would hide under the parameter's own range
        p0 = t["p"].astype(np.float64)
        grad_ok(host(it[0]) - p0, rp - p0, "f32", what + " update")
        grad_ok(host(it[2]), rm, "f32", what + " exp_avg")
        grad_ok(host(it[3]), rv, "f32", what + " exp_avg_sq")


# ------------------------------------------------------------------------------------------------- kd_scale_by_device_scalar
SC = L.cases_of("scale")


@pytest.mark.parametrize("c", SC, ids=L.ids(SC))
def test_scale_by_device_scalar(K, c):
    inp, ref = L.build(c)
    x = cu(inp["x"]).to(DT[c["dt"]])
    x0 = x.clone()
    K.scale_by_device_scalar_(x, torch.tensor([inp["scale"]], device="cuda"))
    reached(c)
    if inp["scale"] == 1.0:
        assert torch.equal(x, x0)
    else:
        # one fp32 product, rounded once more where the storage is bf16
        assert torch.equal(x, (x0.float() * inp["scale"]).to(DT[c["dt"]])), f"{c['id']}: not x * scale rounded once"
        grad_ok(host(x), ref["y"], c["dt"], c["id"])


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_a_misaligned_workspace_is_refused_and_launches_nothing(K):
    c = next(c for c in PAIR if c["id"] == "pair:kld-nhwc-f32-f32-f32")
    inp, _ = L.build(c)
    s, _ = dev(inp["s"], "f32", "cl")
    t, _ = dev(inp["t"], "f32", "cl")
    vs, (N, Cc, P) = K.view3(s)
    vt, _ = K.view3(t)
    loss = torch.empty((), dtype=torch.float32, device="cuda")
    ws, need = K.loss_workspace(N, Cc, P, s.device)
    big = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    off = C.c_void_p(big.data_ptr() + 4)
    mt = lib().MultiTargets()
    mt.n = 1
    mt.t[0] = vt
    mt.w[0] = 1.0
    out3 = torch.empty(3, dtype=torch.float32, device="cuda")
    calls = {
        "kd_kldiv": lambda: lib().lib().kd_kldiv(C.byref(vs), C.byref(vt), C.c_float(2.0), N, Cc, P, K._ptr(loss), None, C.c_float(1.0), off, need, K.stream_ptr()),
        "kd_jsdiv": lambda: lib().lib().kd_jsdiv(C.byref(vs), C.byref(vt), C.c_float(2.0), N, Cc, P, K._ptr(loss), None, C.c_float(1.0), off, need, K.stream_ptr()),
        "kd_hint_mse": lambda: lib().lib().kd_hint_mse(C.byref(vs), C.byref(vt), C.c_float(19.0), N, Cc, P, K._ptr(loss), None, C.c_float(1.0), off, need, K.stream_ptr()),
        "kd_kldiv_multi": lambda: lib().lib().kd_kldiv_multi(C.byref(vs), C.byref(mt), C.c_float(2.0), None, 255, C.c_float(1.0), C.c_float(1.0), N, Cc, P,
                                                             K._ptr(out3), None, off, need, K.stream_ptr()),
    }
    for fn, call in calls.items():
        before = set_note(K)
        with pytest.raises(lib().KdccError, match="aligned"):
            lib().check(call(), fn)
        assert note() == before, f"{fn}: a refused call noted a kernel"
