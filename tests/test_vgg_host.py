"""CIFAR VGG on the host: the checkpoint contract (keys / shapes / parameter count of the reference's vgg16_bn(num_classes=10) and
vgg19(num_classes=100), tests/golden/vgg_keys.json), all eight constructors through the config, the initialisation rule, a
host-plumbing forward of a reduced net against the reference's own logits (tests/golden/vgg.npz, tools/make_golden_vgg.py), the
groups forward() walks, and the refusals."""
import copy
import json
import os

import pytest
import torch

from _netutil import trainer_config
from _seeded import seeded_fill_, seeded_input
from _wrnref import rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))
FULL = {"vgg16_bn": dict(num_classes=10), "vgg19": dict(num_classes=100)}
SMALL_CFG = [16, "M", 32, "M", 64, 64, "M", 64, "M", 512, "M"]
NAMES = ("vgg11", "vgg11_bn", "vgg13", "vgg13_bn", "vgg16", "vgg16_bn", "vgg19", "vgg19_bn")
CONVS = {"vgg11": 8, "vgg13": 10, "vgg16": 13, "vgg19": 16}


@pytest.fixture
def host_tensors():
    from kdcc_amd import nn_hip
    nn_hip.allow_host_tensors(True)
    yield
    nn_hip.allow_host_tensors(False)


def small(batch_norm, num_classes=100):
    from kdcc_amd.models import cifar_models
    return cifar_models.VGG(cifar_models.make_layers(SMALL_CFG, batch_norm), num_classes=num_classes)


@pytest.mark.parametrize("kind", sorted(FULL))
def test_keys_shapes_and_parameter_count_match_reference(kind):
    from kdcc_amd import nn_hip
    from kdcc_amd.models import cifar_models
    with open(os.path.join(HERE, "golden", "vgg_keys.json")) as f:
        inv = json.load(f)[kind]
    with torch.device("meta"):
        m = getattr(cifar_models, kind)(**FULL[kind])
    assert type(m) is cifar_models.VGG and isinstance(m.features, torch.nn.Sequential)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == inv["keys"]
    assert list(m.state_dict()) == list(inv["keys"])
    assert sum(p.numel() for p in m.parameters()) == inv["num_params"]
    assert (len(inv["keys"]), inv["num_params"]) == ((93, 14728266) if kind == "vgg16_bn" else (34, 20075684))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            assert type(mod) is nn_hip.Conv2dNHWC and mod.bias is not None and mod.kernel_size == (3, 3) and mod.padding == (1, 1)
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert type(mod) is nn_hip.BatchNorm2dNHWC
    pools = [i for i, mod in enumerate(m.features) if isinstance(mod, torch.nn.MaxPool2d)]
    assert pools == ([6, 13, 23, 33, 43] if kind == "vgg16_bn" else [4, 9, 18, 27, 36])
    assert sum(isinstance(mod, torch.nn.ReLU) for mod in m.features) == (13 if kind == "vgg16_bn" else 16)
    assert type(m.classifier) is torch.nn.Linear and m.classifier.in_features == 512


@pytest.mark.parametrize("name", NAMES)
def test_every_constructor_resolves_through_the_config(name, tmp_path):
    from kdcc_amd import ConfigParser
    from kdcc_amd.models import cifar_models
    cfgd = trainer_config([], lr=0.1, len_epoch=2, save_dir=str(tmp_path))
    cfgd["teacher"] = {"type": name, "args": {"num_classes": 10}}
    with torch.device("meta"):
        net = ConfigParser(cfgd, run_id=name).init_obj("teacher", cifar_models)
        assert getattr(cifar_models, name)().classifier.out_features == 1000
    assert type(net) is cifar_models.VGG and net.classifier.out_features == 10
    groups = net.features.groups()
    assert len(groups) == CONVS[name.split("_")[0]] and sum(g[3] is not None for g in groups) == 5
    assert all((g[1] is not None) == name.endswith("_bn") and g[2] is not None for g in groups)
    assert [m for g in groups for m in g if m is not None] == list(net.features)


def test_initialisation_rule():
    from kdcc_amd.models import cifar_models
    torch.manual_seed(0)
    m = cifar_models.vgg11_bn(num_classes=10)
    for n, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert bool((mod.weight == 1).all()) and bool((mod.bias == 0).all()), n
        if isinstance(mod, torch.nn.Conv2d):
            assert bool((mod.bias == 0).all()), n
    w = m.features[8].weight.detach()               # normal(0, sqrt(2 / (k k out))), 256 * 128 * 9 samples
    assert tuple(w.shape) == (256, 128, 3, 3) and abs(float(w.std()) / (2.0 / (9 * 256)) ** 0.5 - 1) < 0.05 and abs(float(w.mean())) < 1e-3
    assert abs(float(m.classifier.weight.detach().std()) / 0.01 - 1) < 0.1 and bool((m.classifier.bias == 0).all())


def test_host_forward_of_a_reduced_net_matches_the_reference(golden, host_tensors):
    g = golden("vgg")
    m = small(True)
    seeded_fill_(m, "vgg.host.")
    m.eval()
    x = seeded_input("vgg.host.x", (2, 3, 32, 32))
    with torch.no_grad():
        got = m(x)
        assert rel_l2(got, g["host:logits"]) <= 1e-5
        h = x
        for child in m.features:
            h = child(h)
        assert torch.equal(got, m.classifier(h.flatten(1))), "the walk in groups computes what the children do one by one"
        assert torch.equal(copy.deepcopy(m)(x), got)
    for kind, bn in (("bn", True), ("plain", False)):
        t = small(bn)
        seeded_fill_(t, "vgg.")
        t.eval()
        xs = seeded_input("vgg.x", (8, 3, 32, 32))
        with torch.no_grad():
            assert rel_l2(t(xs), g[f"{kind}:teacher_logits"]) <= 1e-5
        s = copy.deepcopy(t).train()
        if kind == "plain":     # (the goldens' plain student has weights of its own: a copy of the teacher would give a zero loss)
            seeded_fill_(s, "vgg.student.")
        out = s(xs)
        assert rel_l2(out.detach(), g[f"{kind}:student_logits"]) <= 1e-5
        for k, v in s.state_dict().items():
            if "running" in k:
                assert rel_l2(v, g[f"{kind}:stat:" + k]) <= 1e-5, k
            if k.endswith("num_batches_tracked"):
                assert int(v) == 1, k


def test_hooks_fire_with_the_right_operands(host_tensors):
    """A hook on a conv sees the conv's output with the bias added; the pool reads relu(bn(.)) of it."""
    m = small(True, 10).eval()
    seeded_fill_(m, "vgg.host.")
    names = ("features.0", "features.1", "features.2", "features.3", "features.4", "features.11", "features")
    seen = {}
    for name in names:
        m.get_submodule(name).register_forward_hook(lambda mod, i, o, name=name: seen.__setitem__(name, (i[0], o)))
    x = seeded_input("vgg.host.x", (2, 3, 32, 32))
    with torch.no_grad():
        out = m(x)
        assert set(seen) == set(names) and torch.equal(out, m.classifier(seen["features"][1].flatten(1)))
        assert torch.equal(seen["features"][0], x) and tuple(seen["features"][1].shape) == (2, 512, 1, 1)
        f = m.features
        raw = torch.nn.functional.conv2d(x, f[0].weight, f[0].bias, padding=1)
        assert torch.equal(seen["features.0"][1], raw) and torch.equal(seen["features.1"][0], raw)
        act = torch.relu(f[1](raw))
        assert torch.equal(seen["features.3"][0], act) and torch.equal(seen["features.3"][1], torch.nn.functional.max_pool2d(act, 2, 2))
        assert torch.equal(seen["features.4"][0], seen["features.3"][1]) and tuple(seen["features.11"][1].shape) == (2, 64, 8, 8)


def test_refusals():
    from kdcc_amd import nn_hip
    from kdcc_amd._lib import KdccError
    nn_hip.allow_host_tensors(False)
    m = small(True, 10).eval()
    with pytest.raises(KdccError), torch.no_grad():
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(TypeError), torch.no_grad():
        m(torch.zeros(1, 3, 32, 32, dtype=torch.bfloat16))
    f = m.features
    with pytest.raises(KdccError):
        nn_hip.bn_relu_maxpool(f[1], f[2], f[3], torch.zeros(1, 16, 32, 32))
