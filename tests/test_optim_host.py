"""CPU: kdcc_amd.utils.optim resolves what the reference's utils.optim resolves.  SGD / Adam on host tensors ARE torch.optim's
(bit for bit, state dicts cross both ways); AdamW / PlainRAdam on host tensors match the reference's own runs
(tests/golden/optim.npz, tools/make_golden_optim.py); the float64 restatement the GPU tests compare against (_optim_cases.py)
agrees with torch.optim run in float64."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import _optim_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")


@pytest.fixture(scope="module")
def optim():
    import kdcc_amd  # noqa: F401
    from kdcc_amd.utils import optim
    return optim


def test_names_resolve(optim):
    from kdcc_amd.utils.optim import radam, sgd_adam
    assert optim.RAdam is radam.RAdam and optim.PlainRAdam is radam.PlainRAdam and optim.AdamW is radam.AdamW
    assert optim.SGD is sgd_adam.SGD and optim.Adam is sgd_adam.Adam
    assert issubclass(optim.SGD, torch.optim.SGD) and issubclass(optim.Adam, torch.optim.Adam)
    assert optim.AdamW is not torch.optim.AdamW and not issubclass(optim.AdamW, torch.optim.AdamW)
    assert optim.Adagrad is torch.optim.Adagrad                      # the rest of torch.optim is still there
    assert optim.lr_scheduler.__name__.endswith("utils.optim.lr_scheduler")


def test_adamw_takes_the_reference_arguments(optim):
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.AdamW([p], warmup=4)
    assert opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup=4)
    opt = optim.PlainRAdam([p], lr=0.1, degenerated_to_sgd=False)
    assert opt.degenerated_to_sgd is False and opt.defaults["lr"] == 0.1
    for cls in (optim.AdamW, optim.PlainRAdam):
        for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0))):
            with pytest.raises(ValueError):
                cls([p], **bad)


def test_the_entry_point_is_bound(optim):
    from kdcc_amd import _lib, ops
    assert {"kd_optim_step_multi", "kd_optim_launch_shape"} <= set(_lib.exported_symbols()) and callable(ops.optim_step_multi)
    assert ops.optim_step_multi("sgd", []) is None
    p = torch.zeros(4)
    with pytest.raises(_lib.KdccError):                             # host tensors: there is no CPU fallback below the classes
        ops.optim_step_multi("sgd", [(p, p.clone(), (), 0, 0, (0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0))])


def test_case_table_constants_are_the_kernels(optim):
    """The sizes and tensor counts the GPU cases are built round are the library's own (kd_optim_launch_shape)."""
    from kdcc_amd import ops
    assert {r: ops.optim_launch_shape(r) for r in O.MAXT} == {r: (O.MAXT[r], O.OPT_BLK) for r in O.MAXT}
    assert {c[1] for c in O.CASES} == set(O.MAXT)
    src = open(os.path.join(CSRC, "optim.hip")).read()
    assert sorted(set(re.findall(r'KD_NOTE_PLUMBING\("([^"]+)"\)', src))) == [f"optim_multi_kernel<{r}>" for r in sorted(O.MAXT)]


@pytest.mark.parametrize("tag, cls, kw", [("plain", "PlainRAdam", {}), ("plain_nosgd", "PlainRAdam", dict(degenerated_to_sgd=False)),
                                          ("adamw", "AdamW", dict(warmup=4))])
def test_reference_goldens_on_host_tensors(optim, golden, tag, cls, kw):
    g = golden("optim")
    if "warmup" in kw:
        assert int(g["warmup"]) == kw["warmup"]
    p = torch.from_numpy(g[f"{tag}.p"][0].copy()).requires_grad_(True)
    opt = getattr(optim, cls)([p], lr=float(g["lr"]), weight_decay=float(g["weight_decay"]), **kw)
    for i in range(g[f"{tag}.g"].shape[0]):
        p.grad = torch.from_numpy(g[f"{tag}.g"][i].copy())
        opt.step()
        np.testing.assert_allclose(p.detach().numpy(), g[f"{tag}.p"][i + 1], rtol=2e-6, atol=1e-7, err_msg=f"{tag} step {i + 1}")
    st = opt.state[p]
    assert st["step"] == 8 and isinstance(st["step"], int) and set(st) == {"step", "exp_avg", "exp_avg_sq"}
    # the float64 restatement of the same rule, against the same reference run (fp32 there: its own rounding is the bar's)
    rule = "adamw_ref" if cls == "AdamW" else "plain_radam"
    p64, _ = O.run64(rule, dict(lr=float(g["lr"]), weight_decay=float(g["weight_decay"]), **kw), [g[f"{tag}.p"][0]], [list(g[f"{tag}.g"])], steps=8)
    np.testing.assert_allclose(p64[0], g[f"{tag}.p"][8], rtol=2e-6, atol=1e-7)


def test_plain_radam_is_radam_bit_for_bit(optim):
    g = torch.Generator().manual_seed(3)
    a = torch.randn(257, generator=g).requires_grad_(True)
    b = a.detach().clone().requires_grad_(True)
    oa, ob = optim.RAdam([a], lr=0.01, weight_decay=1e-2), optim.PlainRAdam([b], lr=0.01, weight_decay=1e-2)
    for _ in range(8):
        a.grad = torch.randn(257, generator=g)
        b.grad = a.grad.clone()
        oa.step(), ob.step()
    assert torch.equal(a, b)


def _torch_cls(rule):
    return {"sgd": torch.optim.SGD, "adam": torch.optim.Adam}[rule]


def _ours(optim, rule):
    return {"sgd": optim.SGD, "adam": optim.Adam}[rule]


TORCH_CASES = [c for c in O.CASES if c[1] in ("sgd", "adam")]
SMALL = [1, 3, 4, 7, 33]


@pytest.mark.parametrize("cid, rule, kw", TORCH_CASES, ids=[c[0] for c in TORCH_CASES])
def test_host_tensors_step_exactly_as_torch(optim, cid, rule, kw):
    p0, gs = O.inputs(11, SMALL, steps=5)
    a = [torch.from_numpy(p.copy()).requires_grad_(True) for p in p0]
    b = [torch.from_numpy(p.copy()).requires_grad_(True) for p in p0]
    oa, ob = _ours(optim, rule)(a, **kw), _torch_cls(rule)(b, **kw)
    for s in range(5):
        for i in range(len(a)):
            a[i].grad = torch.from_numpy(gs[i][s].copy())
            b[i].grad = torch.from_numpy(gs[i][s].copy())
        oa.step(), ob.step()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        sx, sy = oa.state[x], ob.state[y]
        assert set(sx) == set(sy)
        for k in sx:
            assert type(sx[k]) is type(sy[k]) and torch.equal(torch.as_tensor(sx[k]), torch.as_tensor(sy[k])), k


@pytest.mark.parametrize("cid, rule, kw", TORCH_CASES, ids=[c[0] for c in TORCH_CASES])
def test_float64_restatement_is_torch_in_float64(cid, rule, kw):
    """Only the association inside an element differs, in float64: a few 1e-16 per operation over 20 steps."""
    p0, gs = O.inputs(12, SMALL)
    ps = [torch.from_numpy(p.astype(np.float64)).requires_grad_(True) for p in p0]
    opt = _torch_cls(rule)(ps, **kw)
    for s in range(O.STEPS):
        for i, p in enumerate(ps):
            p.grad = torch.from_numpy(gs[i][s].astype(np.float64))
        opt.step()
    p64, st64 = O.run64(rule, kw, p0, gs)
    for p, q, st in zip(ps, p64, st64):
        np.testing.assert_allclose(q, p.detach().numpy(), rtol=1e-12, atol=1e-13)
        for k in O.STATE_KEYS[rule]:
            assert (k in st) == (k in opt.state[p])
            if k in st:
                np.testing.assert_allclose(st[k], opt.state[p][k].numpy(), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("rule, kw", [("sgd", dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-3)),
                                      ("adam", dict(lr=0.01, amsgrad=True, weight_decay=1e-3))])
@pytest.mark.parametrize("ours_first", [True, False])
def test_state_dict_crosses_between_ours_and_torch(optim, rule, kw, ours_first):
    p0, gs = O.inputs(13, [5, 33], steps=6)

    def fresh(cls):
        ps = [torch.from_numpy(p.copy()).requires_grad_(True) for p in p0]
        return ps, cls(ps, **kw)

    def run(ps, opt, steps):
        for s in steps:
            for i, p in enumerate(ps):
                p.grad = torch.from_numpy(gs[i][s].copy())
            opt.step()

    first, second = (_ours(optim, rule), _torch_cls(rule)) if ours_first else (_torch_cls(rule), _ours(optim, rule))
    pa, oa = fresh(first)
    run(pa, oa, range(3))
    pb, ob = fresh(second)
    with torch.no_grad():
        for x, y in zip(pb, pa):
            x.copy_(y)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    run(pa, oa, range(3, 6))
    run(pb, ob, range(3, 6))
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    for i in sa["state"]:
        for k in sa["state"][i]:
            assert torch.equal(sa["state"][i][k], sb["state"][i][k]), k


@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_add_param_group_with_its_own_hyper_parameters(optim, rule):
    kw0, kw1 = (dict(lr=0.05, momentum=0.9), dict(lr=0.5, momentum=0.5)) if rule == "sgd" else (dict(lr=0.01), dict(lr=0.1, betas=(0.8, 0.9)))
    p0, gs = O.inputs(14, [9, 17], steps=4)
    runs = []
    for cls in (_ours(optim, rule), _torch_cls(rule)):
        ps = [torch.from_numpy(p.copy()).requires_grad_(True) for p in p0]
        opt = cls(ps[:1], **kw0)
        for s in range(4):
            if s == 2:
                opt.add_param_group(dict(params=ps[1:], **kw1))
            for i, p in enumerate(ps):
                p.grad = torch.from_numpy(gs[i][s].copy())
            opt.step()
        assert opt.param_groups[1]["lr"] == kw1["lr"] and len(opt.param_groups) == 2
        runs.append(ps)
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert not np.array_equal(runs[0][1].detach().numpy(), p0[1])


def test_step_hooks_run_once_on_the_torch_path(optim):
    """The fall-back calls torch's step itself, not the hooked wrapper torch installs on torch.optim.SGD once one exists."""
    torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)     # makes torch wrap torch.optim.SGD.step
    p = torch.nn.Parameter(torch.ones(2))
    opt = optim.SGD([p], lr=0.1)
    calls = []
    opt.register_step_post_hook(lambda *a: calls.append(1))
    p.grad = torch.ones(2)
    opt.step()
    assert calls == [1] and torch.equal(p.detach(), torch.full((2,), 0.9))


@pytest.mark.parametrize("rule, kw", [("sgd", dict(lr=0.05, momentum=0.9)), ("adam", dict(lr=0.01))])
def test_a_closure_runs_before_the_step_looks_at_gradients(optim, rule, kw):
    runs = []
    for cls in (_ours(optim, rule), _torch_cls(rule)):
        p = torch.nn.Parameter(torch.arange(6.0))
        opt = cls([p], **kw)

        def closure():
            opt.zero_grad()
            loss = (p * p).sum()
            loss.backward()
            return loss

        losses = [float(opt.step(closure).detach()) for _ in range(3)]
        runs.append((p.detach().clone(), losses))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert not torch.equal(runs[0][0], torch.arange(6.0)) and runs[0][1][1] < runs[0][1][0]
