"""Wide-ResNet CIFAR path on the GPU: kd_bn_nhwc_* against torch's BatchNorm2d, a reduced WRN and two ClassificationTrainer
plans against the reference's own outputs (tests/golden/wrn.npz, tools/make_golden_wrn.py), and WRN-28-10 at full width
against the stock-torch restatement in tests/_wrnref.py."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _netutil import trainer_config  # noqa: E402
from _seeded import seeded_fill_, seeded_input  # noqa: E402
from _wrnref import project, rel_l2, wrn_forward  # noqa: E402

SMALL = dict(depth=10, widen_factor=4, num_classes=100)
PLANS = {
    "c1": {"hint": ["block3.layer.0"], "unfreeze": ["block3.layer.0"], "pruning_plan": ["block3.layer.0.conv2"]},
    "c5": {"hint": ["block3"], "unfreeze": ["block2"], "pruning_plan": ["block2.layer.0.conv2"]},
}


# ------------------------------------------------------------------------------------------------ kd_bn_nhwc_fwd / _bwd
def _bn_case(C, shape, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    N, H, W = shape
    x = torch.randn((N, C, H, W), generator=g) * 1.5 + offset + torch.randn((1, C, 1, 1), generator=g)
    gy = torch.randn((N, C, H, W), generator=g)
    res = torch.randn((N, C, H, W), generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.1 + offset, torch.rand(C, generator=g) + 0.5
    return x, gy, res, gamma, beta, rm, rv


def _torch_bn(x, gy, res, gamma, beta, rm, rv, training, relu):
    """fp64 torch CPU BatchNorm2d (+ ReLU) forward / backward; dx + res."""
    bn = torch.nn.BatchNorm2d(x.shape[1]).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    bn.train(training)
    xd = x.double().requires_grad_(True)
    y = bn(xd)
    if relu:
        y = torch.relu(y)
    y.backward(gy.double())
    return y.detach(), xd.grad + res.double(), bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var


def _dev_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _close(got, ref, tol=1e-5, what=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max().clamp_min(1e-30))
    assert err <= tol * scale, f"{what}: max abs error {err:.3e} > {tol} * {scale:.3e}"


@pytest.mark.parametrize("C", [16, 160, 640])
@pytest.mark.parametrize("shape", [(128, 8, 8), (3, 7, 5), (3, 11, 13)], ids=["128x8x8", "3x7x5", "3x11x13"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
def test_bn_nhwc_matches_torch(C, shape, training, relu):
    from kdcc_amd import ops
    with_res = relu != training
    x, gy, res, gamma, beta, rm, rv = _bn_case(C, shape, seed=C + shape[0])
    y_r, dx_r, dg_r, db_r, rm_r, rv_r = _torch_bn(x, gy, res if with_res else torch.zeros_like(res), gamma, beta, rm, rv,
                                                  training, relu)
    xh = _dev_nhwc(x)
    rmd, rvd = rm.cuda(), rv.cuda()
    y, mean, invstd = ops.bn_nhwc_fwd(xh, gamma.cuda(), beta.cuda(), rmd, rvd, training, 0.1, 1e-5, relu)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dx = ops.bn_nhwc_bwd(_dev_nhwc(gy), xh, y, gamma.cuda(), mean, invstd, training, relu,
                         res=_dev_nhwc(res) if with_res else None, dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    _close(y.permute(0, 3, 1, 2), y_r, what="y")
    _close(dx.permute(0, 3, 1, 2), dx_r, what="dx")
    _close(dg, dg_r, what="dgamma")
    _close(db, db_r, what="dbeta")
    _close(rmd, rm_r, what="running_mean")
    _close(rvd, rv_r, what="running_var")


def test_bn_nhwc_large_mean_and_strided_views():
    """mean ~ 100 std (an fp32 E[x^2] - E[x]^2 would lose the variance), input and output channel slices of wider buffers.
    No ReLU here: at this offset a y within an ulp of 0 may take either side, and its gradient with it."""
    from kdcc_amd import ops
    C = 160
    x, gy, res, gamma, beta, rm, rv = _bn_case(C, (128, 8, 8), seed=7, offset=150.0)
    y_r, dx_r, dg_r, db_r, rm_r, rv_r = _torch_bn(x, gy, torch.zeros_like(res), gamma, beta, rm, rv, True, False)
    wide = torch.zeros((128, 8, 8, C + 32), device="cuda")
    wide[..., 16:16 + C] = _dev_nhwc(x)
    xh = wide[..., 16:16 + C]
    yw = torch.zeros((128, 8, 8, C + 64), device="cuda")
    y, mean, invstd = ops.bn_nhwc_fwd(xh, gamma.cuda(), beta.cuda(), None, None, True, 0.1, 1e-5, False, out=yw[..., 32:32 + C])
    dg = torch.empty(C, device="cuda")
    dx = ops.bn_nhwc_bwd(_dev_nhwc(gy), xh, y, gamma.cuda(), mean, invstd, True, False, dgamma=dg)
    torch.cuda.synchronize()
    var = x.double().var(dim=(0, 2, 3), unbiased=False)
    _close(invstd, 1.0 / torch.sqrt(var + 1e-5), what="invstd")
    _close(y.permute(0, 3, 1, 2), y_r, what="y")
    _close(dx.permute(0, 3, 1, 2), dx_r, what="dx")
    _close(dg, dg_r, what="dgamma")
    assert float(yw[..., :32].abs().max()) == 0.0 and float(yw[..., 32 + C:].abs().max()) == 0.0


def test_bn_nhwc_running_stats_three_steps_and_bitwise():
    from kdcc_amd import nn_hip
    C = 320
    bn_t = torch.nn.BatchNorm2d(C)
    bn = nn_hip.BatchNorm2dNHWC(C).cuda()
    xs = [torch.randn((16, C, 8, 8), generator=torch.Generator().manual_seed(40 + i)) * 2 + 3 for i in range(3)]
    for x in xs:
        bn_t(x)
        bn(x.cuda().contiguous(memory_format=torch.channels_last))
    _close(bn.running_mean, bn_t.running_mean, what="running_mean")
    _close(bn.running_var, bn_t.running_var, what="running_var")
    assert int(bn.num_batches_tracked) == 3

    def run():
        torch.manual_seed(0)
        x = xs[0].cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        b = nn_hip.BatchNorm2dNHWC(C).cuda()
        y = b(x, relu=True)
        y.backward(torch.ones_like(y) * torch.linspace(-1, 1, C, device="cuda").view(1, C, 1, 1))
        return y.detach().clone(), x.grad.clone(), b.weight.grad.clone(), b.running_var.clone()
    a, b = run(), run()
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------ module paths
def test_fused_eval_after_training_sees_current_running_stats():
    """eval (fused, no autograd) -> one train-mode step -> eval again: the folded BN scale / shift of the conv epilogues must
    follow the running statistics the train-mode forward updated, frozen BNs (weights unchanged) included."""
    from kdcc_amd.models.cifar_models import wrn
    m = wrn(depth=16, widen_factor=2, num_classes=10)
    seeded_fill_(m, "wrn.stale.")
    m = m.cuda()
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith("block3"))
    x = seeded_input("wrn.stale.x", (4, 3, 32, 32)).cuda()
    m.eval()
    with torch.no_grad():
        before = m(x)
    m.train()
    m(x * 2.0 + 0.5).sum().backward()
    m.eval()
    with torch.no_grad():
        fused = m(x)
    unfused = m(x).detach()                           # autograd on: the module path, BN from the current buffers
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ref = wrn_forward(sd, x.cpu(), depth=16)
    assert rel_l2(unfused.cpu(), ref) <= 1e-4
    assert rel_l2(fused.cpu(), ref) <= 1e-4
    assert rel_l2(before.cpu(), ref) > 1e-3            # (the statistics did move)


def test_train_mode_gradients_through_identity_shortcuts():
    """depth 16: blocks of equal width, whose identity-shortcut gradient joins bn1's dx in kd_bn_nhwc_bwd (`res`), against
    fp64 autograd of tests/_wrnref.py."""
    from kdcc_amd.models.cifar_models import wrn
    m = wrn(depth=16, widen_factor=2, num_classes=10)
    seeded_fill_(m, "wrn.res.")
    sd = {k: v.clone().double().requires_grad_(v.is_floating_point() and "running" not in k)
          for k, v in m.state_dict().items()}
    m = m.cuda().train()
    assert m.block2.layer[1].equalInOut and m.block2.layer[1].convShortcut is None
    x = seeded_input("wrn.res.x", (4, 3, 32, 32))
    wout = seeded_input("wrn.res.w", (4, 10))
    (m(x.cuda()) * wout.cuda()).sum().backward()
    (wrn_forward(sd, x.double(), depth=16, training=True) * wout.double()).sum().backward()
    # (train-mode BN backward at this size is ill-conditioned: stock torch in fp32 on the CPU lands 2-5e-3 from fp64 on the
    # BN parameters; a lost or doubled shortcut gradient is an O(1) error)
    for n, p in m.named_parameters():
        assert rel_l2(p.grad.cpu(), sd[n].grad) <= 1e-2, n


# ------------------------------------------------------------------------------------------------ reduced WRN vs the reference
def test_small_wrn_matches_reference(golden):
    from kdcc_amd import losses
    from kdcc_amd.models.cifar_models import wrn
    g = golden("wrn")
    teacher = wrn(**SMALL)
    seeded_fill_(teacher, "wrn.")
    teacher = teacher.cuda().eval()
    x = seeded_input("wrn.x", (8, 3, 32, 32)).cuda()
    with torch.no_grad():
        t = teacher(x)
    assert rel_l2(t.cpu(), g["teacher_logits"]) <= 1e-3
    student = copy.deepcopy(teacher).train()
    s = student(x)
    loss = losses.KLDivergenceLoss(temperature=5)(s, t)
    loss.backward()
    assert rel_l2(s.detach().cpu(), g["student_logits"]) <= 1e-3
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=1e-3)
    for k, v in student.state_dict().items():
        if "running" in k:
            assert rel_l2(v.cpu(), g["stat:" + k]) <= 1e-3, k
    for n, p in student.named_parameters():
        assert rel_l2(project(p.grad, n), g["grad:" + n]) <= 1e-3, n


def _wrn_config(plan, save_dir):
    cfgd = trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
    cfgd.update(name="golden_wrn", teacher={"type": "wrn", "args": dict(SMALL)}, optimizer={"type": "SGD", "args": {"lr": 0.1}},
                kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
                hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}},
                metrics=["accuracy", "top_k_acc"],
                lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}})
    cfgd["trainer"]["name"] = "ClassificationTrainer"
    cfgd["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3},
                       **{k: [{"name": n, "epoch": 1} for n in v] for k, v in PLANS[plan].items()}}
    return cfgd


@pytest.mark.parametrize("plan", ["c1", "c5"])
def test_small_wrn_trainer_epoch_matches_reference(golden, tmp_path, plan):
    from kdcc_amd import ConfigParser, losses
    from kdcc_amd.models import cifar_models, metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer import ClassificationTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    g = golden("wrn")
    config = ConfigParser(_wrn_config(plan, str(tmp_path)), run_id=plan)
    teacher = config.init_obj("teacher", cifar_models)
    seeded_fill_(teacher, "wrn.")
    teacher = teacher.cuda().eval()
    model = DepthwiseStudent(teacher, config)
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            blk = model.get_block(b["name"], model.student)
            seeded_fill_(blk, f"wrn.student.{b['name']}.")
    model.replace = replace_and_seed
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    batches = [(seeded_input(f"wrn.tr.x{i}", (8, 3, 32, 32)),
                torch.randint(0, 100, (8,), generator=torch.Generator().manual_seed(300 + i))) for i in range(3)]
    tr = ClassificationTrainer(model, crit, metrics, opt, config, batches, None, sched, WeightScheduler(config["weight_scheduler"]))
    log = tr._train_epoch(1)
    trainable = sorted(n for n, p in model.student.named_parameters() if p.requires_grad)
    assert trainable == list(g[f"{plan}:trainable"])
    for k in ("loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss"):
        np.testing.assert_allclose(log[k], float(g[f"{plan}:log:{k}"]), rtol=2e-3, atol=1e-6, err_msg=k)
    for n, p in model.student.named_parameters():
        if p.requires_grad:
            assert rel_l2(project(p.data, n), g[f"{plan}:param:{n}"]) <= 1e-3, n


# ------------------------------------------------------------------------------------------------ WRN-28-10 at full width
@pytest.fixture(scope="module")
def wrn28():
    from kdcc_amd.models.cifar_models import wrn
    m = wrn(depth=28, widen_factor=10, num_classes=100)
    seeded_fill_(m, "wrn28.")
    return m


def test_wrn28_eval_logits_match_stock_torch(wrn28):
    x = seeded_input("wrn28.x", (4, 3, 32, 32))
    sd = {k: v.clone() for k, v in wrn28.state_dict().items()}
    ref = wrn_forward(sd, x, depth=28)
    m = copy.deepcopy(wrn28).cuda().eval()
    with torch.no_grad():
        got = m(x.cuda())
    assert rel_l2(got.cpu(), ref) <= 1e-3
    got2 = m(x.cuda())                   # autograd on: the unfused module path
    assert rel_l2(got2.detach().cpu(), ref) <= 1e-3


def test_wrn28_student_teacher_bitwise_and_classes(wrn28, tmp_path):
    from kdcc_amd import ConfigParser, nn_hip
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    cfgd = _wrn_config("c1", str(tmp_path))
    config = ConfigParser(cfgd, run_id="w28")
    model = DepthwiseStudent(copy.deepcopy(wrn28).cuda(), config)
    x = seeded_input("wrn28.x", (4, 3, 32, 32)).cuda()
    model.eval()
    with torch.no_grad():
        assert torch.equal(model.student(x), model.teacher(x))
    model.replace([{"name": "block3.layer.0.conv2", "epoch": 1}, {"name": "block3.layer.1.conv2", "epoch": 1}],
                  kernel_size=3, padding=1, dilation=1)
    for net in (model.teacher, model.student):
        for name, m in net.named_modules():
            inside_dw = any(name.startswith(r + ".") for r in model.replaced_block_names) and net is model.student
            if isinstance(m, torch.nn.Conv2d) and not inside_dw:
                assert type(m) is nn_hip.Conv2dNHWC, name
            if isinstance(m, torch.nn.BatchNorm2d):
                assert type(m) is nn_hip.BatchNorm2dNHWC, name
    assert isinstance(model.student.block3.layer[0].conv2, DepthwiseSeparableBlock)


def test_wrn28_training_step_bitwise(wrn28):
    from kdcc_amd import losses
    x = seeded_input("wrn28.x", (4, 3, 32, 32)).cuda()
    teacher = copy.deepcopy(wrn28).cuda().eval()
    with torch.no_grad():
        t = teacher(x)

    def step():
        s = copy.deepcopy(wrn28).cuda().train()
        for n, p in s.named_parameters():
            p.requires_grad_(n.startswith("block3") or n.startswith("block2.layer.3"))
        opt = torch.optim.SGD([p for p in s.parameters() if p.requires_grad], lr=0.1)
        loss = losses.KLDivergenceLoss(temperature=5)(s(x), t)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        return loss.detach(), {k: v.detach().clone() for k, v in s.state_dict().items()}
    l1, a = step()
    l2, b = step()
    assert torch.equal(l1, l2)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["block3.layer.0.conv1.weight"], wrn28.state_dict()["block3.layer.0.conv1.weight"].cuda())
