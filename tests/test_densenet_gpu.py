"""CIFAR DenseNet path on the GPU: the dense_ops kernels (kd_bn_nhwc_stats / _apply, kd_avgpool2x2_nhwc[_bwd]) and
bn_nhwc_bwd(out=) against fp64 torch, the concat-free dense block, a reduced DenseNet and a ClassificationTrainer epoch against
the reference's own outputs (tests/golden/densenet.npz, tools/make_golden_densenet.py -- every bound is max(1e-3, 3 x the
reference's measured fp32-vs-fp64 error of that tensor)), and DenseNet-121 at full width against tests/_densenetref.py."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _densenetref import DENSENET121, SMALL, bound, densenet_forward, project, rel_l2  # noqa: E402
from _netutil import trainer_config  # noqa: E402
from _seeded import seeded_fill_, seeded_input  # noqa: E402

PLAN = ["features.denseblock1.denselayer1.conv2", "features.denseblock1.denselayer2.conv2"]


# ------------------------------------------------------------------------------------------------ kd_bn_nhwc_stats / _apply
def _bn_case(C, shape, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    N, H, W = shape
    x = torch.randn((N, C, H, W), generator=g) * 1.5 + offset + torch.randn((1, C, 1, 1), generator=g)
    gy = torch.randn((N, C, H, W), generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.1 + offset, torch.rand(C, generator=g) + 0.5
    return x, gy, gamma, beta, rm, rv


def _torch_bn(x, gy, gamma, beta, rm, rv, relu):
    """fp64 torch CPU train-mode BatchNorm2d (+ ReLU) forward / backward."""
    bn = torch.nn.BatchNorm2d(x.shape[1]).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    bn.train()
    xd = x.double().requires_grad_(True)
    y = bn(xd)
    if relu:
        y = torch.relu(y)
    y.backward(gy.double())
    return y.detach(), xd.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var


def _dev_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _close(got, ref, tol=1e-5, what=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max().clamp_min(1e-30))
    assert err <= tol * scale, f"{what}: max abs error {err:.3e} > {tol} * {scale:.3e}"


@pytest.mark.parametrize("C", [32, 96, 1024])
@pytest.mark.parametrize("shape", [(8, 2, 2), (3, 7, 5), (32, 16, 16)], ids=["8x2x2", "3x7x5", "32x16x16"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
def test_bn_stats_apply_matches_torch(C, shape, relu):
    from kdcc_amd import ops
    x, gy, gamma, beta, rm, rv = _bn_case(C, shape, seed=C + shape[0])
    y_r, _, _, _, rm_r, rv_r = _torch_bn(x, gy, gamma, beta, rm, rv, relu)
    xh = _dev_nhwc(x)
    rmd, rvd = rm.cuda(), rv.cuda()
    mean, invstd, var = ops.bn_nhwc_stats(xh, 1e-5)
    y = ops.bn_nhwc_apply(xh, gamma.cuda(), beta.cuda(), mean, invstd, var, rmd, rvd, 0.1, relu)
    torch.cuda.synchronize()
    xd = x.double()
    _close(mean, xd.mean(dim=(0, 2, 3)), what="mean")
    _close(invstd, 1.0 / torch.sqrt(xd.var(dim=(0, 2, 3), unbiased=False) + 1e-5), what="invstd")
    _close(y.permute(0, 3, 1, 2), y_r, what="y")
    _close(rmd, rm_r, what="running_mean")
    _close(rvd, rv_r, what="running_var")


def test_bn_stats_apply_large_mean():
    """mean ~ 100 std: an fp32 E[x^2] - E[x]^2 would lose the variance."""
    from kdcc_amd import ops
    C = 96
    x, gy, gamma, beta, rm, rv = _bn_case(C, (32, 16, 16), seed=7, offset=150.0)
    y_r, _, _, _, rm_r, rv_r = _torch_bn(x, gy, gamma, beta, rm, rv, False)
    xh = _dev_nhwc(x)
    rmd, rvd = rm.cuda(), rv.cuda()
    mean, invstd, var = ops.bn_nhwc_stats(xh, 1e-5)
    y = ops.bn_nhwc_apply(xh, gamma.cuda(), beta.cuda(), mean, invstd, var, rmd, rvd, 0.1, False)
    _close(invstd, 1.0 / torch.sqrt(x.double().var(dim=(0, 2, 3), unbiased=False) + 1e-5), what="invstd")
    _close(y.permute(0, 3, 1, 2), y_r, what="y")
    _close(rmd, rm_r, what="running_mean")
    _close(rvd, rv_r, what="running_var")


def test_bn_stats_apply_on_channel_slices_of_wider_buffers():
    from kdcc_amd import ops
    C, shape = 96, (3, 7, 5)
    x, gy, gamma, beta, rm, rv = _bn_case(C, shape, seed=11)
    y_r = _torch_bn(x, gy, gamma, beta, rm, rv, True)[0]
    wide = torch.zeros((3, 7, 5, C + 64), device="cuda")
    wide[..., 32:32 + C] = _dev_nhwc(x)
    yw = torch.zeros((3, 7, 5, C + 32), device="cuda")
    vec = torch.zeros((3, C + 8), device="cuda")
    mean, invstd, var = ops.bn_nhwc_stats(wide[..., 32:32 + C], 1e-5, vec[0, 4:4 + C], vec[1, 4:4 + C], vec[2, 4:4 + C])
    ops.bn_nhwc_apply(wide[..., 32:32 + C], gamma.cuda(), beta.cuda(), mean, invstd, var, None, None, 0.1, True, out=yw[..., 16:16 + C])
    _close(yw[..., 16:16 + C].permute(0, 3, 1, 2), y_r, what="y")
    _close(mean, x.double().mean(dim=(0, 2, 3)), what="mean")
    assert float(yw[..., :16].abs().max()) == 0.0 and float(yw[..., 16 + C:].abs().max()) == 0.0
    assert float(vec[:, :4].abs().max()) == 0.0 and float(vec[:, 4 + C:].abs().max()) == 0.0
    assert float(wide[..., :32].abs().max()) == 0.0 and float(wide[..., 32 + C:].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(8, 2, 2), (32, 16, 16)], ids=["8x2x2", "32x16x16"])
def test_slice_statistics_are_the_bits_the_prefix_forward_saves(shape):
    """The reduction is per channel and shared (bn_nhwc_core.h): statistics of slice [64:96], computed once when the slice is
    produced, are bitwise what kd_bn_nhwc_fwd saves for channels 64..95 of the prefix [0:96]."""
    from kdcc_amd import ops
    x, _, gamma, beta, _, _ = _bn_case(96, shape, seed=3)
    buf = torch.zeros(shape + (128,), device="cuda")
    buf[..., :96] = _dev_nhwc(x)
    rv_a, rv_b = torch.ones(96, device="cuda"), torch.ones(32, device="cuda")
    _, mean_p, invstd_p = ops.bn_nhwc_fwd(buf[..., :96], gamma.cuda(), beta.cuda(), None, rv_a, True, 0.1, 1e-5)
    mean, invstd, var = ops.bn_nhwc_stats(buf[..., 64:96], 1e-5)
    ops.bn_nhwc_apply(buf[..., 64:96], gamma[64:].cuda(), beta[64:].cuda(), mean, invstd, var, None, rv_b, 0.1, out=torch.empty(shape + (32,), device="cuda"))
    assert torch.equal(mean, mean_p[64:]) and torch.equal(invstd, invstd_p[64:])
    assert torch.equal(rv_b, rv_a[64:])              # (the running update is the shared expression too)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
def test_batchnorm_module_with_supplied_statistics_gradients(relu):
    from kdcc_amd import nn_hip, ops
    C, shape = 96, (3, 7, 5)
    x, gy, gamma, beta, rm, rv = _bn_case(C, shape, seed=21)
    y_r, dx_r, dg_r, db_r, rm_r, rv_r = _torch_bn(x, gy, gamma, beta, rm, rv, relu)
    bn = nn_hip.BatchNorm2dNHWC(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    stats = ops.bn_nhwc_stats(xd.detach().permute(0, 2, 3, 1), bn.eps)
    y = bn(xd, relu=relu, stats=stats)
    y.backward(gy.cuda())
    _close(y, y_r, what="y")
    _close(xd.grad, dx_r, what="dx")
    _close(bn.weight.grad, dg_r, what="dgamma")
    _close(bn.bias.grad, db_r, what="dbeta")
    _close(bn.running_mean, rm_r, what="running_mean")
    _close(bn.running_var, rv_r, what="running_var")
    assert int(bn.num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------ kd_avgpool2x2_nhwc
@pytest.mark.parametrize("shape,pad", [((2, 16, 16, 128), 0), ((3, 7, 5, 36), 0), ((2, 6, 9, 32), 32), ((2, 5, 4, 6), 3)],
                         ids=["2x16x16x128", "3x7x5x36", "ld>C", "scalar-ld>C"])
def test_avgpool2x2_forward_and_backward(shape, pad):
    from kdcc_amd import ops
    N, H, W, C = shape
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn((N, C, H, W), generator=g)
    gy = torch.randn((N, C, H // 2, W // 2), generator=g)
    xd = x.double().requires_grad_(True)
    y_r = torch.nn.functional.avg_pool2d(xd, 2, 2)
    y_r.backward(gy.double())
    xw = torch.zeros((N, H, W, C + pad), device="cuda")
    xw[..., :C] = _dev_nhwc(x)
    yw = torch.zeros((N, H // 2, W // 2, C + pad), device="cuda")
    gw = torch.zeros((N, H // 2, W // 2, C + pad), device="cuda")
    gw[..., pad:] = _dev_nhwc(gy)
    gxw = torch.full((N, H, W, C + pad), 7.0, device="cuda")
    y = ops.avgpool2x2(xw[..., :C], out=yw[..., pad:])
    gx = ops.avgpool2x2_bwd(gw[..., pad:], (H, W), out=gxw[..., :C])
    _close(y.permute(0, 3, 1, 2), y_r, tol=1e-6, what="y")
    _close(gx.permute(0, 3, 1, 2), xd.grad, tol=1e-6, what="gx")
    if pad:
        assert float(yw[..., :pad].abs().max()) == 0.0 and bool((gxw[..., C:] == 7.0).all())
    if H % 2:
        assert float(gx[:, H - 1].abs().max()) == 0.0
    if W % 2:
        assert float(gx[:, :, W - 1].abs().max()) == 0.0
    y2 = ops.avgpool2x2(xw[..., :C])
    assert y2.is_contiguous() and torch.equal(y2, y)


# ------------------------------------------------------------------------------------------------ bn_nhwc_bwd(out=)
def test_bn_nhwc_bwd_out_and_exact_alias_of_res():
    from kdcc_amd import ops
    C, shape = 96, (3, 7, 5)
    x, gy, gamma, beta, _, _ = _bn_case(C, shape, seed=5)
    res = torch.randn(shape + (C,), generator=torch.Generator().manual_seed(6)).cuda()
    xh, gh = _dev_nhwc(x), _dev_nhwc(gy)
    y, mean, invstd = ops.bn_nhwc_fwd(xh, gamma.cuda(), beta.cuda(), None, None, True, 0.1, 1e-5, True)
    want = ops.bn_nhwc_bwd(gh, xh, y, gamma.cuda(), mean, invstd, True, True, res=res)
    wide = torch.zeros(shape + (C + 32,), device="cuda")
    got = ops.bn_nhwc_bwd(gh, xh, y, gamma.cuda(), mean, invstd, True, True, res=res, out=wide[..., :C])
    assert got.data_ptr() == wide.data_ptr() and torch.equal(got, want)
    assert float(wide[..., C:].abs().max()) == 0.0
    wide[..., :C] = res                                            # dx accumulated in place into the gradient it adds
    got = ops.bn_nhwc_bwd(gh, xh, y, gamma.cuda(), mean, invstd, True, True, res=wide[..., :C], out=wide[..., :C])
    assert torch.equal(got, want) and float(wide[..., C:].abs().max()) == 0.0
    with pytest.raises(ValueError, match="overlaps"):
        ops.bn_nhwc_bwd(gh, xh, y, gamma.cuda(), mean, invstd, True, True, res=wide[..., 4:C + 4], out=wide[..., :C])
    with pytest.raises(ValueError, match="overlaps"):
        ops.bn_nhwc_bwd(gh, xh, y, gamma.cuda(), mean, invstd, True, True, out=gh)


# ------------------------------------------------------------------------------------------------ concat-free blocks
@pytest.fixture(scope="module")
def small_net():
    from kdcc_amd.models.cifar_models import DenseNet
    return seeded_fill_(DenseNet(**SMALL), "dn.")


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_dense_block_is_concat_free_and_equals_the_concatenation(small_net, mode):
    m = copy.deepcopy(small_net).cuda()
    x = seeded_input("dn.x", (8, 3, 32, 32))
    sd = {k: v.clone() for k, v in small_net.state_dict().items()}
    taps, seen = {}, {}
    names = [f"features.denseblock{k}{s}" for k in (1, 4) for s in ("", ".denselayer1", ".denselayer2", ".denselayer1.conv2", ".denselayer2.conv2")]
    for name in names:
        m.get_submodule(name).register_forward_hook(lambda mod, i, o, name=name: seen.__setitem__(name, o))
    if mode == "eval":
        m.eval()
        with torch.no_grad():
            m(x.cuda())
        densenet_forward(sd, x, SMALL["block_config"], taps=taps)
    else:
        m.train()
        m(x.cuda())
        densenet_forward(sd, x, SMALL["block_config"], training=True, taps=taps)
    for k, c0 in ((1, 64), (4, 64)):
        blk = f"features.denseblock{k}"
        out = seen[blk]
        ptr = out.untyped_storage().data_ptr()
        assert out.shape[1] == c0 + 64 and out.permute(0, 2, 3, 1).stride(3) == 1
        for j in (1, 2):
            o, c = seen[f"{blk}.denselayer{j}"], seen[f"{blk}.denselayer{j}.conv2"]
            assert o.untyped_storage().data_ptr() == ptr and c.untyped_storage().data_ptr() == ptr
            assert o.data_ptr() == out.data_ptr() and o.shape[1] == c0 + 32 * j and c.shape[1] == 32
            assert c.data_ptr() == out.data_ptr() + 4 * (c0 + 32 * (j - 1))
            assert rel_l2(o.detach().cpu(), taps[f"{blk}.denselayer{j}"]) <= 1e-3, (blk, j)
            assert rel_l2(c.detach().cpu(), taps[f"{blk}.denselayer{j}.conv2"]) <= 1e-3, (blk, j)
        assert rel_l2(out.detach().cpu(), taps[f"{blk}.denselayer2"]) <= 1e-3


def test_block_gradients_with_a_second_consumer_of_a_layer_output(small_net):
    """A hint-style second consumer of denselayer1's output (autograd sums its gradient with the chain's) and a caller-owned
    grad_output: the block's in-place gradient chain must write neither, against fp64 autograd of tests/_densenetref.py."""
    m = copy.deepcopy(small_net).cuda().train()
    blk = m.features.denseblock2
    sd = {k[len("features.denseblock2."):]: v.clone().double().requires_grad_(v.is_floating_point() and "running" not in k)
          for k, v in small_net.state_dict().items() if k.startswith("features.denseblock2.")}
    x = seeded_input("dn.blk.x", (4, 64, 8, 8))
    w1, w2 = seeded_input("dn.blk.w1", (4, 96, 8, 8)), seeded_input("dn.blk.w2", (4, 128, 8, 8))
    seen = {}
    blk.denselayer1.register_forward_hook(lambda mod, i, o: seen.__setitem__("l1", o))
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = blk(xd)
    g2 = w2.cuda().contiguous(memory_format=torch.channels_last)     # handed to autograd as the block output's gradient itself
    keep = g2.clone()
    torch.autograd.backward([(seen["l1"] * w1.cuda()).sum(), out], [None, g2])
    assert torch.equal(g2, keep)
    import torch.nn.functional as F
    xr = x.double().requires_grad_(True)
    cur = xr
    for j in (1, 2):
        p = f"denselayer{j}"
        bn = lambda q, t: F.batch_norm(t, None, None, sd[f"{p}.{q}.weight"], sd[f"{p}.{q}.bias"], True, 0.1, 1e-5)
        h = F.conv2d(F.relu(bn("norm1", cur)), sd[p + ".conv1.weight"])
        cur = torch.cat([cur, F.conv2d(F.relu(bn("norm2", h)), sd[p + ".conv2.weight"], padding=1)], 1)
        if j == 1:
            l1 = cur
    ((l1 * w1.double()).sum() + (cur * w2.double()).sum()).backward()
    assert rel_l2(xd.grad.cpu(), xr.grad) <= 1e-3
    for n, p in blk.named_parameters():
        assert rel_l2(p.grad.cpu(), sd[n].grad) <= 1e-3, n


# ------------------------------------------------------------------------------------------------ reduced DenseNet vs the reference
def test_small_densenet_matches_reference(golden):
    from kdcc_amd import losses
    from kdcc_amd.models.cifar_models import DenseNet
    g = golden("densenet")
    tag = str(g["tag"])
    teacher = seeded_fill_(DenseNet(**SMALL), tag).cuda().eval()
    x = seeded_input(tag + "x", (8, 3, 32, 32)).cuda()
    with torch.no_grad():
        t = teacher(x)
    assert rel_l2(t.cpu(), g["teacher_logits"]) <= bound(g, "teacher_logits")
    student = copy.deepcopy(teacher).train()
    s = student(x)
    loss = losses.KLDivergenceLoss(temperature=5)(s, t)
    loss.backward()
    assert rel_l2(s.detach().cpu(), g["student_logits"]) <= bound(g, "student_logits")
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=bound(g, "loss"))
    for k, v in student.state_dict().items():
        if "running" in k:
            assert rel_l2(v.cpu(), g["stat:" + k]) <= bound(g, "stat:" + k), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    for n, p in student.named_parameters():
        assert rel_l2(project(p.grad, n), g["grad:" + n]) <= bound(g, "grad:" + n), n


def _densenet_config(save_dir):
    cfgd = trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
    cfgd.update(name="golden_densenet", teacher={"type": "DenseNet", "args": dict(SMALL)}, optimizer={"type": "SGD", "args": {"lr": 0.1}},
                kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
                hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}},
                metrics=["accuracy", "top_k_acc"],
                lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}})
    cfgd["trainer"]["name"] = "ClassificationTrainer"
    cfgd["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3},
                       **{k: [{"name": n, "epoch": 1} for n in PLAN] for k in ("hint", "unfreeze", "pruning_plan")}}
    return cfgd


def test_small_densenet_trainer_epoch_matches_reference(golden, tmp_path):
    from kdcc_amd import ConfigParser, losses
    from kdcc_amd.models import cifar_models, metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer import ClassificationTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    g = golden("densenet")
    tag = str(g["tag"])
    config = ConfigParser(_densenet_config(str(tmp_path)), run_id="c4")
    teacher = seeded_fill_(config.init_obj("teacher", cifar_models), tag).cuda().eval()
    model = DepthwiseStudent(teacher, config)
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"{tag}student.{b['name']}.")
    model.replace = replace_and_seed
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    batches = [(seeded_input(f"{tag}tr.x{i}", (8, 3, 32, 32)),
                torch.randint(0, 10, (8,), generator=torch.Generator().manual_seed(300 + i))) for i in range(3)]
    tr = ClassificationTrainer(model, crit, metrics, opt, config, batches, None, sched, WeightScheduler(config["weight_scheduler"]))
    log = tr._train_epoch(1)
    trainable = sorted(n for n, p in model.student.named_parameters() if p.requires_grad)
    assert trainable == list(g["c4:trainable"])
    for k in ("loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss"):
        np.testing.assert_allclose(log[k], float(g[f"c4:log:{k}"]), rtol=bound(g, f"c4:log:{k}", floor=2e-3), atol=1e-6, err_msg=k)
    for n, p in model.student.named_parameters():
        if p.requires_grad:
            assert rel_l2(project(p.data, n), g[f"c4:param:{n}"]) <= bound(g, f"c4:param:{n}"), n


# ------------------------------------------------------------------------------------------------ DenseNet-121 at full width
@pytest.fixture(scope="module")
def dn121():
    from kdcc_amd.models.cifar_models import densenet121
    return seeded_fill_(densenet121(), "dn121.")


def test_densenet121_eval_logits_match_stock_torch(dn121):
    x = seeded_input("dn121.x", (4, 3, 32, 32))
    sd = {k: v.clone() for k, v in dn121.state_dict().items()}
    with torch.no_grad():
        ref = densenet_forward(sd, x, DENSENET121)
    m = copy.deepcopy(dn121).cuda().eval()
    with torch.no_grad():
        got = m(x.cuda())
    assert rel_l2(got.cpu(), ref) <= 1e-3
    got2 = m(x.cuda())                   # autograd on: the unfused module path
    assert rel_l2(got2.detach().cpu(), ref) <= 1e-3


def test_densenet121_student_teacher_bitwise_and_classes(dn121, tmp_path):
    from kdcc_amd import ConfigParser, nn_hip
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    config = ConfigParser(_densenet_config(str(tmp_path)), run_id="d121")
    model = DepthwiseStudent(copy.deepcopy(dn121).cuda(), config)
    x = seeded_input("dn121.x", (4, 3, 32, 32)).cuda()
    model.eval()
    with torch.no_grad():
        assert torch.equal(model.student(x), model.teacher(x))
    model.replace([{"name": n, "epoch": 1} for n in PLAN], kernel_size=3, padding=1, dilation=1)
    for net in (model.teacher, model.student):
        for name, m in net.named_modules():
            inside_dw = any(name.startswith(r + ".") for r in model.replaced_block_names) and net is model.student
            if isinstance(m, torch.nn.Conv2d) and not inside_dw:
                assert type(m) is nn_hip.Conv2dNHWC, name
            if isinstance(m, torch.nn.BatchNorm2d):
                assert type(m) is nn_hip.BatchNorm2dNHWC, name
    for n in PLAN:
        assert isinstance(model.get_block(n, model.student), DepthwiseSeparableBlock)
    model.student.train()
    assert tuple(model.student(x).shape) == (4, 10)          # the replaced conv2s are copied into their slices


def test_densenet121_training_step_bitwise(dn121):
    from kdcc_amd import losses
    x = seeded_input("dn121.x", (4, 3, 32, 32)).cuda()
    teacher = copy.deepcopy(dn121).cuda().eval()
    with torch.no_grad():
        t = teacher(x)

    def step():
        s = copy.deepcopy(dn121).cuda().train()
        for n, p in s.named_parameters():
            p.requires_grad_(n.startswith("features.denseblock4"))
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
    k = "features.denseblock4.denselayer1.conv1.weight"
    assert not torch.equal(a[k], dn121.state_dict()[k].cuda())
