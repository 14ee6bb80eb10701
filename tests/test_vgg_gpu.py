"""CIFAR VGG on the GPU.  First the convolutions at the map sizes no other network here reaches (4x4 and 2x2 at 512 channels, and
the biased 3 -> 64 stem) against float64; then two reduced nets (with and without BatchNorm) and one ClassificationTrainer plan
against the reference's own outputs (tests/golden/vgg.npz, tools/make_golden_vgg.py), the fused eval path against the module path,
the hook fallbacks of the fused BN -> ReLU -> max-pool tail, and vgg16_bn at full size.  The network bars are
tests/test_wrn_gpu.py's and tests/test_preresnet_gpu.py's.

The convolution bars are derived: an fp32 dot product of K terms in any order is off by at most (K - 1) u sum |terms| with
u = 2^-24, on top of one rounding per product and per added bias; the tests take (K + 4) u times the same convolution of the
operands' absolute values, K = 9 Cin for the forward, 9 Cout for the input gradient, N Ho Wo for the weight and bias gradients."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _netutil import trainer_config  # noqa: E402
from _seeded import seeded_fill_, seeded_input  # noqa: E402
from _wrnref import project, rel_l2  # noqa: E402

U = 2.0 ** -24
SMALL_CFG = [16, "M", 32, "M", 64, 64, "M", 64, "M", 512, "M"]
CONV_WEIGHTS = {f"features.{i}.weight" for i in (0, 4, 8, 11, 15, 19)}        # (the convs of the reduced BatchNorm net)
PLAN = {"hint": ["features.11"], "unfreeze": ["features.11"], "pruning_plan": ["features.11"]}


@pytest.fixture(autouse=True)
def fused_tail_at_every_size(request, monkeypatch):
    """The reduced nets' maps are all below nn_hip.POOL_FUSE_MIN_ELEMENTS; these tests are about the fused kernels, so they take them
    at every size (the gate itself: test_the_fused_tail_starts_at_its_measured_size)."""
    from kdcc_amd import nn_hip
    if "measured_size" not in request.node.name:
        monkeypatch.setattr(nn_hip, "POOL_FUSE_MIN_ELEMENTS", 0)


def small(batch_norm, num_classes=100):
    from kdcc_amd.models import cifar_models
    return cifar_models.VGG(cifar_models.make_layers(SMALL_CFG, batch_norm), num_classes=num_classes)


# ------------------------------------------------------------------------------------------------ the small maps first
@pytest.mark.parametrize("shape", [(8, 4, 4, 512, 512), (8, 2, 2, 512, 512), (8, 32, 32, 3, 64)], ids=lambda s: "x".join(map(str, s)))
def test_conv_at_the_small_maps_matches_float64(shape):
    """Conv2dNHWC(3x3, padding 1, bias) at VGG's stage-4 / stage-5 maps and at its stem: forward, input gradient, weight and bias
    gradients against float64 with the derived bars of the module docstring."""
    from kdcc_amd import nn_hip
    N, H, W, Ci, Co = shape
    key = "vgg.conv." + "x".join(map(str, shape))
    conv = nn_hip.Conv2dNHWC(Ci, Co, kernel_size=3, padding=1, bias=True)
    seeded_fill_(conv, key + ".")
    x, gy = seeded_input(key + ".x", (N, Ci, H, W)), seeded_input(key + ".gy", (N, Co, H, W))
    xd = x.double().requires_grad_(True)
    wd, bd = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    ref = F.conv2d(xd, wd, bd, padding=1)
    ref.backward(gy.double())
    xa, wa, ba = (t.detach().abs().requires_grad_(True) for t in (xd, wd, bd))
    mag = F.conv2d(xa, wa, ba, padding=1)
    mag.backward(gy.double().abs())
    conv = conv.cuda()
    xg = x.cuda().to(memory_format=torch.channels_last).requires_grad_(True)
    y = conv(xg)
    y.backward(gy.cuda())
    for what, got, want, K, m in (("forward", y, ref, 9 * Ci, mag), ("input gradient", xg.grad, xd.grad, 9 * Co, xa.grad),
                                  ("weight gradient", conv.weight.grad, wd.grad, N * H * W, wa.grad),
                                  ("bias gradient", conv.bias.grad, bd.grad, N * H * W, ba.grad)):
        err = (got.detach().double().cpu() - want.detach()).abs()
        bound = (K + 4) * U * m.detach()
        print(f"{what}: max error {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, worst ratio {float((err / bound).max()):.3f}")
        assert tuple(got.shape) == tuple(want.shape), what
        assert bool((err <= bound).all()), f"{what}: error exceeds its bound by {float((err - bound).max()):.3e}"


# ------------------------------------------------------------------------------------------------ reduced nets vs the reference
@pytest.mark.parametrize("kind", ["bn", "plain"])
def test_small_vgg_matches_reference(golden, kind):
    from kdcc_amd import _lib, losses
    g = golden("vgg")
    teacher = small(kind == "bn")
    seeded_fill_(teacher, "vgg.")
    teacher = teacher.cuda().eval()
    x = seeded_input("vgg.x", (8, 3, 32, 32)).cuda()
    with torch.no_grad():
        t = teacher(x)
    assert _lib.last_plumbing_kernel() == "pool_fwd_kernel<4>", "the last stage's pool did not run fused"
    assert rel_l2(t.cpu(), g[f"{kind}:teacher_logits"]) <= 1e-3
    student = copy.deepcopy(teacher).train()
    if kind == "plain":     # (without BatchNorm a copy of the teacher would give a zero loss: the goldens' student has weights of its own)
        seeded_fill_(student, "vgg.student.")
    s = student(x)
    assert _lib.last_plumbing_kernel() == "pool_fwd_kernel<4>"
    loss = losses.KLDivergenceLoss(temperature=5)(s, t)
    loss.backward()
    assert rel_l2(s.detach().cpu(), g[f"{kind}:student_logits"]) <= 1e-3
    np.testing.assert_allclose(float(loss.detach()), float(g[f"{kind}:loss"]), rtol=1e-3)
    for k, v in student.state_dict().items():
        if "running" in k:
            assert rel_l2(v.cpu(), g[f"{kind}:stat:" + k]) <= 1e-3, k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    for n, p in student.named_parameters():
        if kind == "bn" and n.endswith(".bias") and p.dim() == 1 and n.replace(".bias", ".weight") in CONV_WEIGHTS:
            # the bias of a conv that feeds a train-mode BatchNorm: the BatchNorm subtracts the batch mean, so this gradient is exactly
            # zero and what either side holds is the rounding of a sum that cancels; both stay below the bar relative to the same
            # sum weighted by the conv's input, the weight gradient
            w = n.replace(".bias", ".weight")
            assert torch.linalg.norm(project(p.grad, n)) <= 1e-3 * torch.linalg.norm(project(student.get_parameter(w).grad, w)), n
            assert np.linalg.norm(g[f"{kind}:grad:" + n]) <= 1e-3 * np.linalg.norm(g[f"{kind}:grad:" + w]), n
            continue
        assert rel_l2(project(p.grad, n), g[f"{kind}:grad:" + n]) <= 1e-3, n


def _config(save_dir):
    cfgd = trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
    cfgd.update(name="golden_vgg", teacher={"type": "vgg16_bn", "args": {"num_classes": 100}},
                optimizer={"type": "SGD", "args": {"lr": 0.1}},
                kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
                hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}},
                metrics=["accuracy", "top_k_acc"],
                lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}})
    cfgd["trainer"]["name"] = "ClassificationTrainer"
    cfgd["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3},
                       **{k: [{"name": n, "epoch": 1} for n in v] for k, v in PLAN.items()}}
    return cfgd


def test_small_vgg_trainer_epoch_matches_reference(golden, tmp_path):
    from kdcc_amd import ConfigParser, losses
    from kdcc_amd.models import metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    from kdcc_amd.trainer import ClassificationTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    g = golden("vgg")
    config = ConfigParser(_config(str(tmp_path)), run_id="plan")
    teacher = small(True)
    seeded_fill_(teacher, "vgg.")
    teacher = teacher.cuda().eval()
    model = DepthwiseStudent(teacher, config)
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"vgg.student.{b['name']}.")
    model.replace = replace_and_seed
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    batches = [(seeded_input(f"vgg.tr.x{i}", (8, 3, 32, 32)),
                torch.randint(0, 100, (8,), generator=torch.Generator().manual_seed(300 + i))) for i in range(3)]
    tr = ClassificationTrainer(model, crit, metrics, opt, config, batches, None, sched, WeightScheduler(config["weight_scheduler"]))
    log = tr._train_epoch(1)
    block = model.student.features[11]
    assert isinstance(block, DepthwiseSeparableBlock) and block.pointwise_conv.bias is not None and block.separable_conv.bias is not None
    trainable = sorted(n for n, p in model.student.named_parameters() if p.requires_grad)
    assert trainable == list(g["plan:trainable"])
    for k in ("loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss"):
        np.testing.assert_allclose(log[k], float(g[f"plan:log:{k}"]), rtol=2e-3, atol=1e-6, err_msg=k)
    for n, p in model.student.named_parameters():
        if p.requires_grad:
            assert rel_l2(project(p.data, n), g[f"plan:param:{n}"]) <= 1e-3, n


# ------------------------------------------------------------------------------------------------ module paths
@pytest.mark.parametrize("kind", ["bn", "plain"])
def test_fused_eval_matches_the_module_path_also_after_a_training_step(kind):
    """eval (fused, no autograd: one launch per conv, the no-BatchNorm pool kernel) against the same net with a no-op hook on every
    child (the module path); then one train-mode step, after which the folded BN scale / shift of the conv epilogues must follow the
    running statistics it moved."""
    from kdcc_amd import _lib
    m = small(kind == "bn", 10)
    seeded_fill_(m, "vgg.stale.")
    m = m.cuda().eval()
    x = seeded_input("vgg.stale.x", (4, 3, 32, 32)).cuda()

    def module_path():
        hs = [c.register_forward_hook(lambda mod, i, o: None) for c in m.features]
        with torch.no_grad():
            out = m(x)
        for h in hs:
            h.remove()
        return out
    with torch.no_grad():
        before = m(x)
    assert _lib.last_plumbing_kernel() == "pool_fwd_kernel<4>"
    assert rel_l2(before.cpu(), module_path().cpu()) <= 1e-4
    assert rel_l2(before.cpu(), m(x).detach().cpu()) <= 1e-4          # autograd on: the fused tail in eval mode
    m.train()
    m(x * 2.0 + 0.5).sum().backward()
    m.eval()
    with torch.no_grad():
        fused = m(x)
    unfused = module_path()
    assert rel_l2(fused.cpu(), unfused.cpu()) <= 1e-4
    assert rel_l2(m(x).detach().cpu(), unfused.cpu()) <= 1e-4
    if kind == "bn":
        assert rel_l2(before.cpu(), unfused.cpu()) > 1e-3              # (the statistics did move)
    else:
        assert torch.equal(before, fused)


def test_a_hook_on_a_conv_sees_its_raw_output_on_either_path():
    m = small(True, 10)
    seeded_fill_(m, "vgg.hook.")
    m = m.cuda().eval()
    x = seeded_input("vgg.hook.x", (2, 3, 32, 32)).cuda()
    with torch.no_grad():
        fused = m(x)
    seen = {}
    for n in ("features.8", "features.11"):
        m.get_submodule(n).register_forward_hook(lambda mod, i, o, n=n: seen.__setitem__(n, (i[0].detach().clone(), o.detach().clone())))
    with torch.no_grad():
        hooked = m(x)
    a = dict(seen)
    seen.clear()
    unfused = m(x).detach()
    f = m.features
    for n in a:
        assert rel_l2(a[n][1].cpu(), seen[n][1].cpu()) <= 1e-4 and rel_l2(a[n][0].cpu(), seen[n][0].cpu()) <= 1e-4, n
    raw = F.conv2d(a["features.11"][0].cpu().double(), f[11].weight.detach().cpu().double(), f[11].bias.detach().cpu().double(), padding=1)
    assert rel_l2(a["features.11"][1].cpu(), raw) <= 1e-4, "the hook sees conv + bias, not the activation"
    assert float(a["features.11"][1].min()) < 0 <= float(a["features.11"][0].min())
    assert rel_l2(hooked.cpu(), fused.cpu()) <= 1e-4 and rel_l2(unfused.cpu(), fused.cpu()) <= 1e-4


@pytest.mark.parametrize("where", ["bn", "relu", "pool", "features"])
def test_a_hooked_tail_falls_back_to_the_modules_with_the_same_results(where):
    """A forward hook on the BatchNorm, the ReLU or the pool of a stage makes nn_hip.bn_relu_maxpool call the modules: same logits
    and gradients, the running statistics bit for bit (one update rule), and the hook sees its module's output."""
    from kdcc_amd import _lib
    base = small(True, 10)
    seeded_fill_(base, "vgg.tail.")
    x = seeded_input("vgg.tail.x", (4, 3, 32, 32)).cuda()
    wout = seeded_input("vgg.tail.w", (4, 10)).cuda()
    idx = {"bn": 5, "relu": 6, "pool": 7}
    runs = {}
    for mode in ("fused", "hooked"):
        m = copy.deepcopy(base).cuda().train()
        seen = []
        if mode == "hooked":
            (m.features if where == "features" else m.features[idx[where]]).register_forward_hook(lambda mod, i, o: seen.append(tuple(o.shape)))
        out = m(x)
        if mode == "fused":
            assert _lib.last_plumbing_kernel() == "pool_fwd_kernel<4>"
        (out * wout).sum().backward()
        want = {"bn": (4, 32, 16, 16), "relu": (4, 32, 16, 16), "pool": (4, 32, 8, 8), "features": (4, 512, 1, 1)}[where]
        assert seen == ([want] if mode == "hooked" else [])
        f = m.features
        runs[mode] = (out.detach(), f[5].weight.grad, f[5].bias.grad, f[4].weight.grad, f[4].bias.grad, f[0].weight.grad, f[19].weight.grad,
                      f[5].running_mean.clone(), f[5].running_var.clone(), int(f[5].num_batches_tracked))
    f, h = runs["fused"], runs["hooked"]
    names = ("logits", "features.5.weight.grad", "features.5.bias.grad", "features.4.weight.grad", "features.4.bias.grad",
             "features.0.weight.grad", "features.19.weight.grad")
    for a, b, what in zip(f[:7], h[:7], names):
        if what == "features.4.bias.grad":      # (exactly zero behind a train-mode BatchNorm: rounding on both sides, see above)
            assert float((a - b).norm()) <= 1e-4 * float(f[3].norm()) and float(a.norm()) <= 1e-4 * float(f[3].norm()), what
            continue
        assert rel_l2(a.cpu(), b.cpu()) <= 1e-4, what
    assert torch.equal(f[7], h[7]) and torch.equal(f[8], h[8]) and f[9] == h[9] == 1
    if where != "features":
        m = copy.deepcopy(base).cuda().eval()
        with torch.no_grad():
            fused = m(x)
            m.features[idx[where]].register_forward_hook(lambda mod, i, o: None)
            assert rel_l2(m(x).cpu(), fused.cpu()) <= 1e-4


def test_reduced_nets_read_the_padded_pooled_map_in_place():
    """The pooled 16-channel map comes from new_padded() and is tagged: the next conv reads its 32-channel granule without a copy."""
    from kdcc_amd import nn_hip
    m = small(True, 10)
    seeded_fill_(m, "vgg.pad.")
    m = m.cuda().train()
    x = seeded_input("vgg.pad.x", (2, 3, 32, 32)).cuda()
    f = m.features
    y = nn_hip.bn_relu_maxpool(f[1], f[2], f[3], f[0](x))
    assert tuple(y.shape) == (2, 16, 16, 16) and y.permute(0, 2, 3, 1).stride(2) == 32
    pre = f[4]._prepadded(y)
    assert pre is not None and pre.data_ptr() == y.data_ptr() and bool((pre[..., 16:] == 0).all())


def test_the_fused_tail_starts_at_its_measured_size():
    """Both sides of nn_hip.POOL_FUSE_MIN_ELEMENTS at batch 128: vgg16_bn's 4x4x512 stage takes the fused kernels, its 2x2x512 stage
    (where they lost to the composition, profiles/vgg.md) bn(x, relu=True) + MaxPool2d; the form without BatchNorm has no gate."""
    from kdcc_amd import _lib, nn_hip
    assert nn_hip.POOL_FUSE_MIN_ELEMENTS == 128 * 4 * 4 * 512
    bn, relu, pool = nn_hip.BatchNorm2dNHWC(512).cuda().train(), torch.nn.ReLU(inplace=True), torch.nn.MaxPool2d(2, 2)
    outs = {}
    # (the backward runs on autograd's own thread, whose plumbing note this thread does not see: the graph node says which one it is)
    for side, first, last in ((4, "pool_fwd_kernel<4>", "_BNReLUMaxPoolFnBackward"), (2, "bn_nhwc_apply_kernel<4>", "MaxPool")):
        x = seeded_input(f"vgg.gate.{side}", (128, 512, side, side)).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        y = nn_hip.bn_relu_maxpool(bn, relu, pool, x)
        assert _lib.last_plumbing_kernel() == first and type(y.grad_fn).__name__.startswith(last), (side, type(y.grad_fn).__name__)
        y.sum().backward()
        assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0, side
        assert tuple(y.shape) == (128, 512, side // 2, side // 2)
        with torch.no_grad():
            nn_hip.bn_relu_maxpool(None, relu, pool, x)
        assert _lib.last_plumbing_kernel() == "pool_fwd_kernel<4>", "no gate without BatchNorm"
        outs[side] = (y.detach(), x.grad.clone(), x.detach())
    y, gx, x = outs[2]                          # the composition computes what the fused kernels do
    ref = F.max_pool2d(F.relu(F.batch_norm(x.double(), None, None, bn.weight.double(), bn.bias.double(), True)), 2, 2)
    assert rel_l2(y.cpu(), ref.cpu()) <= 1e-4


# ------------------------------------------------------------------------------------------------ vgg16_bn at full size
def test_vgg16_bn_trains_one_batch_of_128():
    from kdcc_amd import _lib
    from kdcc_amd.models.cifar_models import vgg16_bn
    torch.manual_seed(0)
    m = vgg16_bn(num_classes=10).cuda().train()
    x = seeded_input("vgg16.x", (128, 3, 32, 32)).cuda()
    out = m(x)
    assert _lib.last_plumbing_kernel() == "pool_fwd_kernel<4>"
    assert tuple(out.shape) == (128, 10) and bool(torch.isfinite(out).all())
    F.cross_entropy(out, torch.arange(128, device="cuda") % 10).backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape) and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    m.eval()
    with torch.no_grad():
        ev = m(x)
    assert tuple(ev.shape) == (128, 10) and bool(torch.isfinite(ev).all())
