"""The optimizer kernels (csrc/optim.hip, kd_optim_step_multi) through the classes of kdcc_amd.utils.optim, on the device.

Bar of the float64 comparisons, measured in the test: the same rule run in fp32 on the CPU by torch (torch.optim.SGD / Adam; for
the reference's AdamW, this package's host path, which is the reference's sequence of torch operations) on the same inputs is the
yardstick; the device result's max and rms deviation from the float64 restatement (_optim_cases.py) must each be at most 2 x the
yardstick's.  Only the association of the products and sums inside one element differs between the two fp32 runs (fused
multiply-adds here, torch's own kernels there): a numpy fp32 restatement in the other association order gave ratios of 1.00 to
1.15 (max) and 1.00 to 1.08 (rms) on 300001 elements over 20 steps, hence the margin of 2.  Nothing here is derived from the
kernel's output."""
import numpy as np
import pytest
import torch

import _optim_cases as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def optim():
    import kdcc_amd  # noqa: F401
    from kdcc_amd.utils import optim
    assert torch.cuda.is_available()
    return optim


def note():
    from kdcc_amd import _lib
    return _lib.last_plumbing_kernel()


def classes(optim, rule):
    """(class under test, fp32 CPU yardstick class)"""
    return {"sgd": (optim.SGD, torch.optim.SGD), "adam": (optim.Adam, torch.optim.Adam), "adamw_ref": (optim.AdamW, optim.AdamW)}[rule]


def make_params(p0, device, offset=()):
    """Parameters holding p0 on `device`; those whose index is in `offset` are views starting one element into their storage
    (4-byte aligned only: the scalar path)."""
    out = []
    for i, p in enumerate(p0):
        t = torch.from_numpy(p.copy()).to(device)
        if i in offset:
            buf = torch.empty(t.numel() + 1, device=device)
            buf[1:].copy_(t)
            t = buf[1:]
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        out.append(torch.nn.Parameter(t))
    return out


def run(cls, kw, p0, gs, device, offset=(), steps=O.STEPS):
    ps = make_params(p0, device, offset)
    opt = cls(ps, **kw)
    for s in range(steps):
        for i, p in enumerate(ps):
            p.grad = None if gs[i][s] is None else torch.from_numpy(gs[i][s]).to(device)
        opt.step()
    return ps, opt


def deviation(got, ref):
    """(max, rms) of got - ref over all tensors together."""
    d = np.concatenate([np.asarray(g, np.float64).ravel() - r.ravel() for g, r in zip(got, ref)])
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


def host(t):
    return t.detach().cpu().numpy()


def hold_to_yardstick(what, dev, cpu, ref):
    (dm, dr), (cm, cr) = deviation(dev, ref), deviation(cpu, ref)
    print(f"{what}: device max {dm:.3e} rms {dr:.3e}; fp32 CPU yardstick max {cm:.3e} rms {cr:.3e}")
    assert dm <= 2 * cm and dr <= 2 * cr, (f"{what}: deviation from float64: device max {dm:.3e} rms {dr:.3e}, "
                                           f"fp32 CPU yardstick max {cm:.3e} rms {cr:.3e} (bar: 2 x the yardstick)")


def against_float64(optim, cid, rule, kw, p0, gs, offset, steps=O.STEPS):
    ours, yard = classes(optim, rule)
    ref_p, ref_s = O.run64(rule, kw, p0, gs, steps)
    dev_p, dev_o = run(ours, kw, p0, gs, "cuda", offset, steps)
    cpu_p, cpu_o = run(yard, kw, p0, gs, "cpu", (), steps)
    hold_to_yardstick(f"{cid} p", [host(p) for p in dev_p], [host(p) for p in cpu_p], ref_p)
    for k in O.STATE_KEYS[rule]:
        idx = [i for i, st in enumerate(ref_s) if k in st]
        assert all((k in dev_o.state[p]) == (i in idx) for i, p in enumerate(dev_p)), f"{cid}: which tensors hold {k}"
        if idx:
            hold_to_yardstick(f"{cid} {k}", [host(dev_o.state[dev_p[i]][k]) for i in idx], [host(cpu_o.state[cpu_p[i]][k]) for i in idx],
                              [ref_s[i][k] for i in idx])
    return dev_p, dev_o


# ------------------------------------------------------------------------------------------ every rule and flag, every size
# the sizes of O.SIZES, then the last two again as views one element into their storage (scalar path), whose values must
# equal their aligned twins' bit for bit
@pytest.mark.parametrize("cid, rule, kw", O.CASES, ids=O.IDS)
def test_rule_against_float64(optim, cid, rule, kw):
    sizes = O.SIZES + O.SIZES[-2:]
    p0, gs = O.inputs(100 + O.IDS.index(cid), O.SIZES)
    p0, gs = p0 + p0[-2:], gs + gs[-2:]
    twins = {len(sizes) - 2: len(O.SIZES) - 2, len(sizes) - 1: len(O.SIZES) - 1}
    ps, opt = against_float64(optim, cid, rule, kw, p0, gs, offset=set(twins))
    assert note() == f"optim_multi_kernel<{rule}>"
    for a, b in twins.items():
        assert ps[a].data_ptr() % 16 == 4 and ps[b].data_ptr() % 16 == 0
        assert torch.equal(ps[a], ps[b]), f"{cid}: the scalar path and the 16-byte path store different values (n = {sizes[a]})"
        for k in O.STATE_KEYS[rule]:
            if k in opt.state[ps[a]]:
                assert torch.equal(opt.state[ps[a]][k], opt.state[ps[b]][k]), f"{cid}: {k} differs between the paths"


# --------------------------------------------------------------------------------------------------- the reference's goldens
@pytest.mark.parametrize("tag, cls, kw", [("plain", "PlainRAdam", {}), ("plain_nosgd", "PlainRAdam", dict(degenerated_to_sgd=False)),
                                          ("adamw", "AdamW", dict(warmup=4))])
def test_reference_goldens_on_the_device(optim, golden, tag, cls, kw):
    g = golden("optim")
    p = torch.nn.Parameter(torch.from_numpy(g[f"{tag}.p"][0].copy()).cuda())
    opt = getattr(optim, cls)([p], lr=float(g["lr"]), weight_decay=float(g["weight_decay"]), **kw)
    for i in range(g[f"{tag}.g"].shape[0]):
        p.grad = torch.from_numpy(g[f"{tag}.g"][i].copy()).cuda()
        opt.step()
        np.testing.assert_allclose(host(p), g[f"{tag}.p"][i + 1], rtol=2e-6, atol=1e-7, err_msg=f"{tag} step {i + 1}")
    assert note() == ("optim_multi_kernel<adamw_ref>" if cls == "AdamW" else "radam_multi_kernel")
    assert opt.state[p]["step"] == 8 and set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"}


# ----------------------------------------------------------------------------------- more tensors than two kernel arguments hold
HP = {"sgd": lambda i: dict(lr=0.01 * (1 + i % 7), momentum=(0.0, 0.5, 0.9)[i % 3], dampening=0.1 * (i % 2), weight_decay=1e-3 * (i % 4)),
      "adam": lambda i: dict(lr=0.002 * (1 + i % 7), betas=(0.9 - 0.1 * (i % 3), 0.999 - 0.01 * (i % 2)), weight_decay=1e-3 * (i % 4),
                             amsgrad=i % 5 == 0),
      "adamw_ref": lambda i: dict(lr=0.002 * (1 + i % 7), betas=(0.9 - 0.1 * (i % 3), 0.999), weight_decay=1e-2 * (i % 4), warmup=(0, 7)[i % 2])}


@pytest.mark.parametrize("rule", sorted(O.MAXT))
def test_chunks_with_their_own_hyper_parameters_and_step_counts(optim, rule):
    """2 * MAXT + 9 tensors, one parameter group each (own lr, betas / momentum, weight decay, warm-up, amsgrad), tensor i joining at
    step i % 4 (own step count, own first-step momentum flag), every third one 4-byte aligned only, sizes that end inside, on and
    past a block: three launches whose chunk boundaries fall between tensors of different constants.  4 steps, so the float64
    bar is the yardstick's again."""
    count, steps = 2 * O.MAXT[rule] + 9, 4
    sizes = [(1, 5, 8, 31, 64, O.OPT_BLK + 3)[i % 6] for i in range(count)]
    p0, gs = O.inputs(7, sizes, steps)
    gs = [[None if s < i % 4 else g for s, g in enumerate(gi)] for i, gi in enumerate(gs)]
    ours, yard = classes(optim, rule)
    offset = set(range(0, count, 3))

    def grouped(cls, device, off):
        ps = make_params(p0, device, off)
        opt = cls([dict(params=[p], **HP[rule](i)) for i, p in enumerate(ps)])
        for s in range(steps):
            for i, p in enumerate(ps):
                p.grad = None if gs[i][s] is None else torch.from_numpy(gs[i][s]).to(device)
            opt.step()
        return ps, opt

    dev_p, dev_o = grouped(ours, "cuda", offset)
    cpu_p, _ = grouped(yard, "cpu", ())
    ref_p = []
    for i in range(count):
        q, _ = O.run64(rule, HP[rule](i), [p0[i]], [gs[i]], steps)
        ref_p.append(q[0])
    hold_to_yardstick(f"{rule} x {count}", [host(p) for p in dev_p], [host(p) for p in cpu_p], ref_p)
    # per tensor as well: a constant taken from a neighbour would move one small tensor by far more than its own rounding, and
    # could hide in the statistics of all of them
    for i in range(count):
        (dm, _), (cm, _) = deviation([host(dev_p[i])], [ref_p[i]]), deviation([host(cpu_p[i])], [ref_p[i]])
        # (a tensor of a few elements can have a yardstick deviation of exactly 0: four steps, each of which rounds the parameter
        # once and carries in under half an ulp from the state, are allowed 4 ulp of the largest parameter)
        slack = 4 * float(np.spacing(np.float32(np.abs(ref_p[i]).max())))
        assert dm <= 2 * cm + slack, f"{rule} tensor {i} ({sizes[i]} elements, {HP[rule](i)}): device {dm:.3e}, yardstick {cm:.3e}"
    if rule != "sgd":
        want = [steps - i % 4 for i in range(count)]
        assert [int(dev_o.state[p]["step"]) for p in dev_p] == want


def test_a_parameter_that_joins_at_step_3(optim):
    """Its momentum buffer is born at step 3 (buf = g) while its neighbours' are two steps old."""
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-3)
    p0, gs = O.inputs(21, [O.OPT_BLK + 1, 37, 300])
    gs[1] = [None, None] + gs[1][2:]
    ps, opt = against_float64(optim, "sgd-late", "sgd", kw, p0, gs, offset=(), steps=6)
    assert set(opt.state[ps[1]]) == {"momentum_buffer"}


# ------------------------------------------------------------------------------------------------- alone and among 100 others
@pytest.mark.parametrize("rule, kw", [("sgd", dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-3)),
                                      ("adam", dict(lr=0.01, amsgrad=True, weight_decay=1e-3)),
                                      ("adamw_ref", dict(lr=0.01, warmup=7, weight_decay=1e-2))])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
def test_alone_and_among_100_others_is_the_same(optim, rule, kw, aligned):
    ours, _ = classes(optim, rule)
    n, steps = O.OPT_BLK + 7, 3
    p0, gs = O.inputs(31, [n] + [(3, 16, 65, 1000)[i % 4] for i in range(100)], steps)
    alone_p, alone_o = run(ours, kw, p0[:1], gs[:1], "cuda", () if aligned else {0}, steps)
    order = list(range(1, 51)) + [0] + list(range(51, 101))            # the tensor sits in the middle of the second launch
    among_p, among_o = run(ours, kw, [p0[i] for i in order], [gs[i] for i in order], "cuda", () if aligned else {50}, steps)
    a, b = alone_p[0], among_p[50]
    assert a.data_ptr() % 16 == b.data_ptr() % 16 == (0 if aligned else 4)
    assert torch.equal(a, b)
    for k in O.STATE_KEYS[rule]:
        assert torch.equal(alone_o.state[a][k], among_o.state[b][k]), k


# ------------------------------------------------------------------------------------------------------- which path is taken
def test_kernel_log_names_the_step(optim):
    def one_step(cls, **kw):
        p = torch.nn.Parameter(torch.ones(10, device="cuda"))
        opt = cls([p], **kw)
        p.grad = torch.ones(10, device="cuda")
        opt.step()
        return note()

    assert one_step(optim.SGD, lr=0.1) == "optim_multi_kernel<sgd>"
    assert one_step(optim.Adam) == "optim_multi_kernel<adam>"
    assert one_step(optim.AdamW, warmup=2) == "optim_multi_kernel<adamw_ref>"
    assert one_step(optim.PlainRAdam) == "radam_multi_kernel"
    assert one_step(optim.RAdam) == "radam_kernel"


@pytest.mark.parametrize("rule, kw", [("sgd", dict(lr=0.05, momentum=0.9)), ("adam", dict(lr=0.01))])
@pytest.mark.parametrize("kind", ["bf16", "non-contiguous"])
def test_other_tensors_take_the_torch_path(optim, rule, kw, kind):
    ours, theirs = classes(optim, rule)
    src = torch.randn(6, 10, generator=torch.Generator().manual_seed(5))
    grads = [torch.randn(6, 10, generator=torch.Generator().manual_seed(6 + s)) for s in range(3)]

    def make(t):
        t = t.cuda()
        return torch.nn.Parameter(t.bfloat16() if kind == "bf16" else t.t())      # the transposed view is not contiguous

    good = torch.randn(8, generator=torch.Generator().manual_seed(9))
    runs, before = [], make(src).detach().clone()
    for cls in (ours, theirs):
        ps = [make(src), torch.nn.Parameter(good.clone().cuda())]
        assert (ps[0].dtype == torch.bfloat16) if kind == "bf16" else not ps[0].is_contiguous()
        opt = cls(ps, **kw)
        for s in range(3):
            ps[0].grad = make(grads[s]).detach()
            ps[1].grad = torch.full((8,), 0.5, device="cuda")
            opt.step()
        runs.append(ps)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], before)


def test_ops_refuses_what_it_cannot_step(optim):
    from kdcc_amd import _lib, ops
    hp = (0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    p, g = torch.zeros(4, 6, device="cuda"), torch.zeros(4, 6, device="cuda")
    with pytest.raises(TypeError):
        ops.optim_step_multi("sgd", [(p.bfloat16(), g.bfloat16(), (), 0, 0, hp)])
    with pytest.raises(TypeError):
        ops.optim_step_multi("sgd", [(p.t(), g.t(), (), 0, 0, hp)])
    with pytest.raises(_lib.KdccError):
        ops.optim_step_multi("sgd", [(p, g.cpu(), (), 0, 0, hp)])
    with pytest.raises(_lib.KdccError):                                    # adam without its state
        ops.optim_step_multi("adam", [(p, g, (), 1, 0, hp)])
    assert torch.equal(p, torch.zeros_like(p))


@pytest.mark.parametrize("rule, kw", [("sgd", dict(lr=0.05, momentum=0.9)), ("adam", dict(lr=0.01)), ("adamw_ref", dict(lr=0.01))])
def test_a_parameter_without_a_gradient_is_left_alone(optim, rule, kw):
    ours, _ = classes(optim, rule)
    a = torch.nn.Parameter(torch.ones(9, device="cuda"))
    b = torch.nn.Parameter(torch.ones(9, device="cuda"))
    opt = ours([a, b], **kw)
    for _ in range(2):
        a.grad = torch.ones(9, device="cuda")
        opt.step()
    assert torch.equal(b, torch.ones_like(b)) and len(opt.state[b]) == 0 and not torch.equal(a, torch.ones_like(a))
    b.grad = torch.ones(9, device="cuda")
    opt.step()
    if rule != "sgd":
        assert int(opt.state[a]["step"]) == 3 and int(opt.state[b]["step"]) == 1
    else:
        assert set(opt.state[b]) == {"momentum_buffer"} and torch.equal(opt.state[b]["momentum_buffer"], b.grad)


# ---------------------------------------------------------------------------------------------------------------- closures
@pytest.mark.parametrize("rule, kw", [("sgd", dict(lr=0.05, momentum=0.9)), ("adam", dict(lr=0.01))])
def test_gradients_that_exist_only_after_the_closure_are_stepped(optim, rule, kw):
    """zero_grad(); backward() inside the closure: before it every gradient is None.  The first step(closure) must already move p,
    on the kernel, and three steps must match torch.optim on the device to a few fp32 roundings of a parameter of magnitude up to
    6 (one ulp there is 4.8e-7; each step rounds p once)."""
    ours, theirs = classes(optim, rule)
    runs = []
    for cls in (ours, theirs):
        p = torch.nn.Parameter(torch.arange(1.0, 7.0, device="cuda"))
        opt = cls([p], **kw)

        def closure():
            opt.zero_grad()
            loss = (p * p).sum()
            loss.backward()
            return loss

        first = float(opt.step(closure).detach())
        after_one = p.detach().clone()
        if cls is ours:
            assert note() == f"optim_multi_kernel<{rule}>"
        for _ in range(2):
            last = float(opt.step(closure).detach())
        runs.append((after_one, p.detach().clone(), first, last))
        if rule == "adam":
            assert int(opt.state[p]["step"]) == 3
    assert runs[0][2] == runs[1][2] == 91.0 and runs[0][3] < 91.0
    assert not torch.equal(runs[0][0], torch.arange(1.0, 7.0, device="cuda")), "the first step(closure) stepped nothing"
    assert (runs[0][0] - runs[1][0]).abs().max().item() <= 4.8e-7 and (runs[0][1] - runs[1][1]).abs().max().item() <= 3 * 4.8e-7


@pytest.mark.parametrize("rule, kw", [("sgd", dict(lr=0.05, momentum=0.9)), ("adam", dict(lr=0.01))])
def test_an_empty_parameter_is_torchs_no_op(optim, rule, kw):
    ours, _ = classes(optim, rule)
    e = torch.nn.Parameter(torch.empty(0, 3, device="cuda"))
    p = torch.nn.Parameter(torch.ones(5, device="cuda"))
    opt = ours([e, p], **kw)
    e.grad, p.grad = torch.empty(0, 3, device="cuda"), torch.ones(5, device="cuda")
    opt.step()
    assert e.numel() == 0 and not torch.equal(p, torch.ones_like(p))
