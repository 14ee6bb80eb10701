"""The CIFAR Wide-ResNet in bf16: nn_hip.Conv2dNHWC / BatchNorm2dNHWC on bf16 channels-last tensors, models/cifar_models/wrn.py
through both its paths, and the public switch of DepthwiseStudent.

Convolutions (3->16, 16->160 3x3, 160->320 3x3 stride 2, 160->320 1x1 stride 2: forward with residual, input gradient, weight
gradient) are held to float64 on the bf16-rounded operands with the bf16 bars of tests/test_ops_gpu.py::assert_close.

Networks (depth 10 widen 4; depth 16 widen 2, whose blocks keep their width: identity shortcuts) have no fixed bar.  Each quantity --
eval logits fused and unfused, train-mode logits, every running statistic, every parameter gradient -- is compared with the exact
float64 network (tests/_wrnref.wrn_forward), and its rel_l2 must be at most 2 x the rel_l2 of tests/_wrn_bf16_ref.py's emulation (the
same float64 network rounding to bf16 where the kernels store bf16) against the same exact result, computed here from the reference
alone.  Kernels and emulation round at the same points but accumulate in different orders; hence the 2.  A floor of 1e-6 is added to
the bar: what the device computes in fp32 behind the last bf16 tensor (pool, fc, the gradient of fc.bias, which no rounding point
feeds) the emulation computes in float64 with an error of zero, and 1e-6 is what fp32 sums of this length give.

The trainer epoch (plan c1 of tests/test_wrn_gpu.py, with the key trainer.dtype = "bf16") is compared with the reference's logged
losses in tests/golden/wrn.npz.  The bar per loss is 2 x |emulated epoch - golden| plus the bar the fp32 path has for the same
figures (rtol 2e-3, atol 1e-6: tests/test_wrn_gpu.py), since the golden is a float32 run of other code.  The emulated epoch with its
roundings switched off reproduces the golden itself (checked on the CPU below)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _wrn_bf16_ref as E
from _netutil import trainer_config
from _seeded import seeded_fill_, seeded_input
from _wrnref import rel_l2, wrn_forward

BF = torch.bfloat16
gpu = pytest.mark.gpu
NETS = {"d10w4": dict(depth=10, widen_factor=4, num_classes=10), "d16w2": dict(depth=16, widen_factor=2, num_classes=10)}
SMALL = dict(depth=10, widen_factor=4, num_classes=100)
C1 = {"hint": ["block3.layer.0"], "unfreeze": ["block3.layer.0"], "pruning_plan": ["block3.layer.0.conv2"]}
FLOOR = 1e-6
LOSSES = ("loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss")


def cl(t, dtype=BF):
    return t.cuda().to(dtype=dtype, memory_format=torch.channels_last)


# --------------------------------------------------------------------------------------------------------------- Conv2dNHWC
CONVS = [(3, 16, 3, 1), (16, 160, 3, 1), (160, 320, 3, 2), (160, 320, 1, 2)]


@gpu
@pytest.mark.parametrize("case", CONVS, ids=lambda c: "%d-%d-k%d-s%d" % c)
def test_conv_bf16_forward_with_residual_and_both_gradients(case):
    from kdcc_amd import nn_hip
    from test_ops_gpu import assert_close
    cin, cout, k, s = case
    g = torch.Generator().manual_seed(cin * 1000 + cout + k)
    conv = nn_hip.Conv2dNHWC(cin, cout, k, stride=s, padding=k // 2, bias=False).cuda()
    N, H = 4, 16
    Ho = (H + 2 * (k // 2) - k) // s + 1
    x, w = torch.randn(N, cin, H, H, generator=g).to(BF), (torch.randn(conv.weight.shape, generator=g) / (cin * k * k) ** 0.5).to(BF)
    res, gy = torch.randn(N, cout, Ho, Ho, generator=g).to(BF), torch.randn(N, cout, Ho, Ho, generator=g).to(BF)
    with torch.no_grad():
        conv.weight.copy_(w.float())
    xd = cl(x).requires_grad_(True)
    y = conv(xd, residual=cl(res))
    y.backward(cl(gy))
    assert y.dtype == BF and xd.grad.dtype == BF and conv.weight.grad.dtype == torch.float32 and conv.weight.dtype == torch.float32
    assert y.is_contiguous(memory_format=torch.channels_last)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    (F.conv2d(x64, w64, stride=s, padding=k // 2) + res.double()).backward(gy.double())
    ref = F.conv2d(x64, w64, stride=s, padding=k // 2) + res.double()
    what = "conv %d->%d k%d s%d" % case
    assert_close(y.detach().float().cpu().numpy(), ref.detach().numpy(), "bf16", what + " forward + residual")
    assert_close(xd.grad.float().cpu().numpy(), x64.grad.numpy(), "bf16", what + " input gradient")
    assert_close(conv.weight.grad.cpu().numpy(), w64.grad.numpy(), "bf16", what + " weight gradient")
    # the packed weights are cached per dtype: an fp32 call afterwards packs its own and computes in fp32
    y32 = conv(cl(x, torch.float32), residual=cl(res, torch.float32))
    assert y32.dtype == torch.float32
    assert_close(y32.detach().cpu().numpy(), ref.detach().numpy(), "f32", what + " fp32 after bf16")


@gpu
def test_batchnorm_module_bf16_output_is_read_in_place_by_the_next_conv(monkeypatch):
    """BatchNorm2dNHWC's bf16 output lives in a buffer zero-padded to the 64-channel K granule and says so; the conv behind it makes
    no padding copy.  A 16- and a 160-channel tensor: read at 64 and at 192 channels."""
    from kdcc_amd import nn_hip
    copies = []
    orig = nn_hip._nhwc_padded
    monkeypatch.setattr(nn_hip, "_nhwc_padded", lambda t, cpad: (copies.append((t.shape[1], cpad)), orig(t, cpad))[1])
    for C, cpad in ((16, 64), (160, 192)):
        bn, conv = nn_hip.BatchNorm2dNHWC(C).cuda().train(), nn_hip.Conv2dNHWC(C, 32, 3, padding=1, bias=False).cuda()
        x = cl(torch.randn(2, C, 8, 8, generator=torch.Generator().manual_seed(C)))
        a = bn(x, relu=True)
        assert a.dtype == BF and getattr(a, nn_hip._PADDED) == cpad and a.permute(0, 2, 3, 1).stride(2) == cpad
        view = conv._input(a)
        assert tuple(view.shape) == (2, 8, 8, cpad) and view.data_ptr() == a.data_ptr() and not bool(view[..., C:].any())
        y = conv(a)
        assert copies == [] and y.dtype == BF
        ref = F.conv2d(a.detach().double().cpu(), conv.weight.detach().to(BF).double().cpu(), padding=1)
        assert rel_l2(y.detach().float().cpu(), ref) <= 5e-3
        conv(x)                                            # an untagged tensor is copied into a zeroed buffer
        assert copies == [(C, cpad)]
        copies.clear()


@gpu
def test_run_folded_bf16_applies_the_eval_batchnorm_in_the_epilogue_and_leaves_the_zero_tail():
    from kdcc_amd import nn_hip
    conv, bn = nn_hip.Conv2dNHWC(16, 160, 3, padding=1, bias=False).cuda(), seeded_fill_(nn_hip.BatchNorm2dNHWC(160), "wrn.bf16.fold.").cuda().eval()
    x = cl(seeded_input("wrn.bf16.fold.x", (2, 16, 8, 8)))
    with torch.no_grad():
        y = conv.run_folded(x, bn, relu=True)
    assert y.dtype == BF and getattr(y, nn_hip._PADDED) == 192
    wide = nn_hip.Conv2dNHWC(160, 64, 1, bias=False).cuda()._input(y)
    assert tuple(wide.shape) == (2, 8, 8, 192) and wide.data_ptr() == y.data_ptr() and not bool(wide[..., 160:].any())
    ref = F.relu(F.batch_norm(F.conv2d(x.double().cpu(), conv.weight.detach().to(BF).double().cpu(), padding=1), bn.running_mean.double().cpu(),
                              bn.running_var.double().cpu(), bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), False, 0.1, bn.eps))
    assert rel_l2(y.float().cpu(), ref) <= 5e-3          # (one bf16 store: ~1.1e-3 rms, tests/test_ops_gpu.py)
    with pytest.raises(TypeError, match="is fp32"):      # the any-channel-count subclass stays fp32-only
        nn_hip.Conv2dNHWCBias(64, 48, 1).cuda()(cl(torch.zeros(1, 64, 4, 4)))
    with pytest.raises(TypeError, match="is fp32"):
        nn_hip.AvgPool2x2NHWC(2, 2)(cl(torch.zeros(1, 64, 4, 4)))


# ------------------------------------------------------------------------------------------------------- the reduced networks
@functools.lru_cache(maxsize=None)
def net_ref(key):
    """The seeded network, its batch, and per quantity: the exact float64 value and the emulation's rel_l2 against it."""
    from kdcc_amd.models.cifar_models import wrn
    kw = NETS[key]
    m = seeded_fill_(wrn(**kw), f"wrn.bf16.{key}.")
    depth = kw["depth"]
    x, w = seeded_input(f"wrn.bf16.{key}.x", (8, 3, 32, 32)), seeded_input(f"wrn.bf16.{key}.w", (8, kw["num_classes"]))
    exact, emul = {}, {}
    frozen = {k: v.detach() for k, v in E.double_sd(m).items()}
    exact["eval"] = wrn_forward(frozen, x.double(), depth=depth)
    emul["eval unfused"] = E.Net(depth).forward(frozen, x.double()).detach()
    emul["eval fused"] = E.Net(depth).forward_fused(frozen, x.double())

    def train(forward):
        sd = E.double_sd(m)
        out = forward(sd)
        (out * w.double()).sum().backward()
        q = {"train logits": out.detach()}
        q.update({"stat:" + k: v.detach() for k, v in sd.items() if "running" in k})
        q.update({"grad:" + k: v.grad for k, v in sd.items() if v.requires_grad})
        return q
    ex = train(lambda sd: wrn_forward(sd, x.double(), depth=depth, training=True))
    em = train(lambda sd: E.Net(depth).forward(sd, x.double(), training=True))
    exact.update(ex)
    err = {k: rel_l2(emul[k], exact["eval"]) for k in emul}
    err.update({k: rel_l2(em[k], ex[k]) for k in ex})
    return m, x, w, exact, err


def held(got, exact, emul_err, what):
    err = rel_l2(got.detach().double().cpu(), exact)
    print(f"BF16ERR {what}: kernels {err:.3e}  emulation {emul_err:.3e}")
    return None if err <= 2 * emul_err + FLOOR else f"{what}: rel_l2 {err:.3e} > 2 x {emul_err:.3e} + {FLOOR}"


@gpu
@pytest.mark.parametrize("key", sorted(NETS))
def test_reduced_wrn_eval_logits_fused_and_unfused(key):
    m, x, w, exact, emul = net_ref(key)
    net = copy.deepcopy(m).cuda().eval()
    xb = cl(x)
    with torch.no_grad():
        fused = net(xb)
    unfused = net(xb)                   # autograd on: the module path
    assert fused.dtype == unfused.dtype == torch.float32
    missed = [held(fused, exact["eval"], emul["eval fused"], f"{key} eval logits, fused"),
              held(unfused, exact["eval"], emul["eval unfused"], f"{key} eval logits, unfused")]
    assert not any(missed), [s for s in missed if s]
    with torch.no_grad():
        assert torch.equal(fused, net(xb)), "the fused path is not bit-reproducible"


@gpu
@pytest.mark.parametrize("key", sorted(NETS))
def test_reduced_wrn_train_logits_statistics_and_every_gradient(key):
    m, x, w, exact, emul = net_ref(key)
    net = copy.deepcopy(m).cuda().train()
    out = net(cl(x))
    (out * w.cuda()).sum().backward()
    assert out.dtype == torch.float32
    missed = [held(out, exact["train logits"], emul["train logits"], f"{key} train logits")]
    for k, v in net.state_dict().items():
        if "running" in k:
            assert v.dtype == torch.float32
            missed.append(held(v, exact["stat:" + k], emul["stat:" + k], f"{key} {k}"))
    for n, p in net.named_parameters():
        assert p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32, n
        missed.append(held(p.grad, exact["grad:" + n], emul["grad:" + n], f"{key} grad {n}"))
    assert not any(missed), [s for s in missed if s]


# ------------------------------------------------------------------------------------------------------- DepthwiseStudent
def wrn_config(save_dir, dtype=None):
    """tests/test_wrn_gpu.py's plan c1; dtype=None leaves the key trainer.dtype out, as the reference's JSON files do."""
    cfgd = trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
    cfgd.update(name="golden_wrn", teacher={"type": "wrn", "args": dict(SMALL)}, optimizer={"type": "SGD", "args": {"lr": 0.1}},
                kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
                hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}},
                metrics=["accuracy", "top_k_acc"],
                lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}})
    cfgd["trainer"]["name"] = "ClassificationTrainer"
    del cfgd["trainer"]["dtype"]
    if dtype is not None:
        cfgd["trainer"]["dtype"] = dtype
    cfgd["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3}, **{k: [{"name": n, "epoch": 1} for n in v] for k, v in C1.items()}}
    return cfgd


def batches():
    return [(seeded_input(f"wrn.tr.x{i}", (8, 3, 32, 32)), torch.randint(0, 100, (8,), generator=torch.Generator().manual_seed(300 + i)))
            for i in range(3)]


@functools.lru_cache(maxsize=None)
def emulated_epoch(emulate):
    """The logged losses of the c1 epoch by tests/_wrn_bf16_ref.py: frozen eval-mode teacher (fused chain), train-mode student with
    block3.layer.0.conv2 replaced and block3.layer.0 unfrozen, KD loss back-propagated, plain SGD at lr 0.1, three batches."""
    from kdcc_amd.models.cifar_models import wrn
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    teacher = seeded_fill_(wrn(**SMALL), "wrn.")
    name = C1["pruning_plan"][0]
    blk = seeded_fill_(DepthwiseSeparableBlock(256, 256, 3, 1, 1, 256, None), f"wrn.student.{name}.")
    cheap = {name: tuple(w.detach().clone().double().requires_grad_(True) for w in (blk.separable_conv.weight, blk.pointwise_conv.weight))}
    tsd = {k: v.detach() for k, v in E.double_sd(teacher).items()}
    ssd = E.double_sd(teacher, trainable=lambda k: k.startswith("block3.layer.0.") and not k.startswith(name + "."))
    ssd.pop(name + ".weight")
    params = [v for v in ssd.values() if v.requires_grad] + list(cheap[name])
    tnet, snet = E.Net(10, emulate, hints=C1["hint"]), E.Net(10, emulate, cheap=cheap, hints=C1["hint"])
    logs = {k: [] for k in LOSSES}
    for x, target in batches():
        t = tnet.forward_fused(tsd, x.double())
        s = snet.forward(ssd, x.double(), training=True)
        kd = E.kld(s, t, 5.0)
        kd.backward()
        with torch.no_grad():
            for p in params:
                p -= 0.1 * p.grad
                p.grad = None
        logs["loss"].append(float(kd.detach())); logs["kd_loss"].append(float(kd.detach()))
        logs["supervised_loss"].append(float(F.cross_entropy(s.detach(), target)))
        logs["teacher_loss"].append(float(F.cross_entropy(t, target)))
        logs["hint_loss"].append(float(F.mse_loss(snet.hints[0].detach(), tnet.hints[0])))
    return {k: float(np.mean(v)) for k, v in logs.items()}


def golden_wrn():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrn.npz"), allow_pickle=False)


def test_the_emulated_epoch_without_rounding_is_the_goldens_epoch():
    """CPU: with every rounding switched off, tests/_wrn_bf16_ref.py walks the reference's epoch (so its bf16 figures measure bf16)."""
    g, e = golden_wrn(), emulated_epoch(False)
    for k in LOSSES:
        np.testing.assert_allclose(e[k], float(g[f"c1:log:{k}"]), rtol=2e-3, atol=1e-6, err_msg=k)


def run_epoch(tmp_path, run_id):
    from kdcc_amd import ConfigParser, losses
    from kdcc_amd.models import cifar_models, metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    from kdcc_amd.trainer import ClassificationTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    config = ConfigParser(wrn_config(str(tmp_path), "bf16"), run_id=run_id)
    teacher = seeded_fill_(config.init_obj("teacher", cifar_models), "wrn.").cuda().eval()
    model = DepthwiseStudent(teacher, config)               # the key alone turns bf16 on
    assert model.module_dtype == BF
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"wrn.student.{b['name']}.")
    model.replace = replace_and_seed
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    tr = ClassificationTrainer(model, crit, metrics, opt, config, batches(), None, sched, WeightScheduler(config["weight_scheduler"]))
    log = tr._train_epoch(1)
    assert isinstance(model.student.block3.layer[0].conv2, DepthwiseSeparableBlock)
    assert all(p.dtype == torch.float32 for p in model.parameters())
    sd = {k: v.detach().clone() for k, v in model.student.state_dict().items()}
    assert all(v.dtype == torch.float32 for v in sd.values() if v.is_floating_point())
    assert [h.dtype for h in model.student_hidden_outputs] == [BF] and [h.dtype for h in model.teacher_hidden_outputs] == [BF]
    # one more backward by hand (the epoch has stepped and cleared its own): the gradients the optimizer is handed are fp32
    s, t = model(batches()[0][0].cuda())
    crit[1](s, t).backward()
    grads = {n: p.grad.dtype for n, p in model.student.named_parameters() if p.grad is not None}
    assert "block3.layer.0.conv2.pointwise_conv.weight" in grads and "block3.layer.0.bn1.weight" in grads
    assert set(grads.values()) == {torch.float32}, "parameter gradients are fp32"
    assert s.dtype == t.dtype == torch.float32
    return log, sd


@gpu
def test_student_switch_bitwise_teacher_and_the_c1_epoch(golden, tmp_path):
    from kdcc_amd.models import cifar_models
    from kdcc_amd.models.students import DepthwiseStudent
    g = golden("wrn")
    teacher = seeded_fill_(cifar_models.wrn(**SMALL), "wrn.").cuda().eval()
    model = DepthwiseStudent(teacher, None, dtype=BF)
    assert model.module_dtype == BF
    x = seeded_input("wrn.x", (8, 3, 32, 32)).cuda()
    model.eval()
    with torch.no_grad():
        s, t = model(x)
        assert s.dtype == t.dtype == torch.float32 and torch.equal(s, t), "student and teacher differ before replace"
        assert torch.equal(model.inference(x), s)
        assert torch.equal(s, model.teacher(cl(x))), "forward does not hand teacher and student the one bf16 channels-last cast"
    log, sd = run_epoch(tmp_path / "a", "bf16a")
    emul = emulated_epoch(True)
    for k in LOSSES:
        ref = float(g[f"c1:log:{k}"])
        bar = 2 * abs(emul[k] - ref) + 2e-3 * abs(ref) + 1e-6
        print(f"BF16ERR c1 epoch {k}: kernels {log[k]:.6f}  emulation {emul[k]:.6f}  golden {ref:.6f}  bar {bar:.3e}")
        assert abs(log[k] - ref) <= bar, f"{k}: {log[k]} vs golden {ref}, bar {bar:.3e} (emulation {emul[k]})"
    log2, sd2 = run_epoch(tmp_path / "b", "bf16b")
    assert all(log[k] == log2[k] for k in LOSSES), "a second identical epoch logs other losses"
    assert all(torch.equal(sd[k], sd2[k]) for k in sd), "a second identical epoch is not bit-identical"


@gpu
def test_without_the_switch_nothing_changes(tmp_path):
    from kdcc_amd import ConfigParser
    from kdcc_amd.models import cifar_models
    from kdcc_amd.models.students import DepthwiseStudent
    teacher = seeded_fill_(cifar_models.wrn(**SMALL), "wrn.").cuda().eval()
    x = seeded_input("wrn.x", (8, 3, 32, 32)).cuda()
    for config in (None, ConfigParser(wrn_config(str(tmp_path)), run_id="nokey")):
        model = DepthwiseStudent(teacher, config)
        assert model.module_dtype == torch.float32 and model.dtype == BF       # (today's ignored default stays what it was)
        model.eval()
        with torch.no_grad():
            s, t = model(x)
            assert torch.equal(s, model.student(x)) and torch.equal(t, model.teacher(x)) and torch.equal(model.inference(x), s)
        model.train()
        s, _ = model(x)
        assert s.dtype == torch.float32 and torch.equal(s.detach(), copy.deepcopy(model.student).train()(x).detach())


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_switch_logic_refusals_and_the_cheap_conv_error_on_the_host():
    from kdcc_amd import models
    from kdcc_amd.models import cifar_models
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    key = lambda v: {"trainer": {"dtype": v}}
    with torch.device("meta"):
        w = cifar_models.wrn(depth=10, widen_factor=1, num_classes=10)
        others = [cifar_models.resnet20(), cifar_models.DenseNet(block_config=(1, 1), num_classes=10)]
    F32 = torch.float32
    for config, dtype, want in ((None, None, F32), ({"trainer": {}}, None, F32), (key("fp32"), None, F32), (key("bf16"), None, BF),
                                (key("bfloat16"), None, BF), (None, BF, BF), (None, F32, F32), (key("bf16"), F32, F32), (key("fp32"), BF, BF)):
        s = DepthwiseStudent(w, config, **({} if dtype is None else {"dtype": dtype}))
        assert s.module_dtype == want, (config, dtype)
        assert not s.fused and not s.engine_plan
        with pytest.raises(AttributeError):
            s.module_dtype = BF
    for net in others:                          # no other module-graph network changes, whatever is asked
        assert DepthwiseStudent(net, key("bf16")).module_dtype == F32 and DepthwiseStudent(net, None, dtype=BF).module_dtype == F32
    s = DepthwiseStudent(w, None, dtype=BF)
    with pytest.raises(RuntimeError, match="GPU only"):
        s(torch.zeros(1, 3, 32, 32))
    # HRNet's refusal is what it was
    from test_hrnet_host import NARROW
    with torch.device("meta"):
        hr = models.HighResolutionNet(copy.deepcopy(NARROW))
    with pytest.raises(TypeError, match="fp32 only"):
        DepthwiseStudent(hr, None, dtype=BF)
    assert DepthwiseStudent(hr, key("bf16")).module_dtype == F32
    # a bf16 cheap-conv block needs 64-channel granules: a clear error, never the fp32 NCHW small-shape kernels
    blk = DepthwiseSeparableBlock(160, 160, 3, 1, 1, 160, None)
    with pytest.raises(ValueError, match="multiples of 64"):
        blk(torch.zeros(1, 160, 8, 8, dtype=BF, device="meta"))
    with pytest.raises(ValueError, match="multiples of 64"):
        DepthwiseSeparableBlock(320, 160, 3, 1, 1, 320, None)(torch.zeros(1, 320, 8, 8, dtype=BF, device="meta"))


def test_the_emulation_without_rounding_is_the_exact_network():
    from kdcc_amd.models.cifar_models import wrn
    for key, kw in NETS.items():
        m = seeded_fill_(wrn(**kw), f"wrn.bf16.{key}.")
        sd = {k: v.detach() for k, v in E.double_sd(m).items()}
        x = seeded_input(f"wrn.bf16.{key}.x", (2, 3, 32, 32)).double()
        ref = wrn_forward(sd, x, depth=kw["depth"])
        net = E.Net(kw["depth"], emulate=False)
        assert torch.equal(net.forward(sd, x), ref) and rel_l2(net.forward_fused(sd, x), ref) <= 1e-12
        assert 1e-4 < rel_l2(E.Net(kw["depth"]).forward(sd, x), ref) < 3e-2          # ... and with it, bf16's distance from it
