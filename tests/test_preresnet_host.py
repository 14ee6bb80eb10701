"""CIFAR PreResNet on the host: the checkpoint contract (keys / shapes / parameter count of the reference's preresnet-110 and
Bottleneck preresnet-164, tests/golden/preresnet_keys.json), the depth refusals, config resolution and a 'module.'-prefixed
checkpoint, a host-plumbing forward against the stock-torch restatement in tests/_preresnetref.py, and the operands hooks see."""
import copy
import json
import os

import pytest
import torch

from _netutil import trainer_config
from _preresnetref import preresnet_forward
from _seeded import seeded_fill_, seeded_input
from _wrnref import rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))
FULL = {"basic": dict(depth=110, num_classes=100), "bottleneck": dict(depth=164, num_classes=100, block_name="Bottleneck")}
SMALL = {"basic": dict(depth=14, num_classes=10), "bottleneck": dict(depth=20, num_classes=10, block_name="Bottleneck")}


@pytest.fixture
def host_tensors():
    from kdcc_amd import nn_hip
    nn_hip.allow_host_tensors(True)
    yield
    nn_hip.allow_host_tensors(False)


@pytest.mark.parametrize("kind", ["basic", "bottleneck"])
def test_keys_shapes_and_parameter_count_match_reference(kind):
    from kdcc_amd import nn_hip
    from kdcc_amd.models import cifar_models
    with open(os.path.join(HERE, "golden", "preresnet_keys.json")) as f:
        inv = json.load(f)[kind]
    with torch.device("meta"):
        m = cifar_models.preresnet(**FULL[kind])
    assert type(m) is cifar_models.PreResNet
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == inv["keys"]
    assert list(m.state_dict()) == list(inv["keys"])
    assert sum(p.numel() for p in m.parameters()) == inv["num_params"]
    if kind == "bottleneck":
        assert len(inv["keys"]) == 983 and inv["num_params"] == 1726388
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            assert type(mod) is nn_hip.Conv2dNHWC
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert type(mod) is nn_hip.BatchNorm2dNHWC
    with_ds = [n for n, b in m.named_modules() if getattr(b, "downsample", None) is not None]
    assert with_ds == (["layer2.0", "layer3.0"] if kind == "basic" else ["layer1.0", "layer2.0", "layer3.0"])
    for n in with_ds:
        ds = m.get_submodule(n).downsample
        assert len(ds) == 1 and ds[0].kernel_size == (1, 1) and ds[0].bias is None
        assert ds[0].stride == ((1, 1) if n == "layer1.0" else (2, 2))
    assert m.fc.in_features == m.bn.num_features == (64 if kind == "basic" else 256)


def test_depth_refusals_match_reference():
    from kdcc_amd.models.cifar_models import preresnet
    with torch.device("meta"):
        with pytest.raises(AssertionError):
            preresnet(depth=21, num_classes=10)
        with pytest.raises(AssertionError):
            preresnet(depth=26, num_classes=10, block_name="Bottleneck")       # 6n+2, not 9n+2
        with pytest.raises(ValueError):
            preresnet(depth=20, num_classes=10, block_name="Wide")
        preresnet(depth=20, num_classes=10, block_name="BASICBLOCK")
        preresnet(depth=20, num_classes=10, block_name="bottleneck")
        assert preresnet(depth=8).fc.out_features == 1000


def test_initialisation_rule():
    from kdcc_amd.models.cifar_models import preresnet
    torch.manual_seed(0)
    m = preresnet(depth=20, num_classes=10, block_name="Bottleneck")
    for n, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert bool((mod.weight == 1).all()) and bool((mod.bias == 0).all()), n
    w = m.layer3[1].conv2.weight.detach()          # normal(0, sqrt(2 / (k k out))), 64 * 64 * 9 samples
    assert abs(float(w.std()) / (2.0 / (9 * 64)) ** 0.5 - 1) < 0.05 and abs(float(w.mean())) < 1e-3


def test_type_resolves_through_config_and_prefixed_checkpoint_loads(tmp_path):
    from kdcc_amd import ConfigParser
    from kdcc_amd.models import cifar_models, forgiving_state_restore
    src = cifar_models.preresnet(**SMALL["basic"])
    seeded_fill_(src, "preresnet.ckpt.")
    ckpt = str(tmp_path / "preresnet.pth")
    torch.save({"state_dict": {"module." + k: v for k, v in src.state_dict().items()}}, ckpt)
    cfgd = trainer_config([], lr=0.1, len_epoch=2, save_dir=str(tmp_path))
    cfgd["teacher"] = {"type": "preresnet", "args": dict(SMALL["basic"]), "snapshot": ckpt}
    config = ConfigParser(cfgd, run_id="p")
    assert type(config.init_obj("teacher", cifar_models)) is cifar_models.PreResNet
    net = config.restore_snapshot("teacher", cifar_models)
    for k, v in src.state_dict().items():
        assert torch.equal(net.state_dict()[k], v), k
    other = cifar_models.preresnet(**SMALL["basic"])
    forgiving_state_restore(other, {"module." + k: v for k, v in src.state_dict().items()})
    assert all(torch.equal(other.state_dict()[k], v) for k, v in src.state_dict().items())


@pytest.mark.parametrize("kind", ["basic", "bottleneck"])
def test_host_forward_matches_stock_torch(kind, host_tensors):
    from kdcc_amd.models import cifar_models
    m = cifar_models.preresnet(**SMALL[kind])
    seeded_fill_(m, "preresnet.host.")
    x = seeded_input("preresnet.host.x", (2, 3, 32, 32))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.eval()
    with torch.no_grad():
        assert rel_l2(m(x), preresnet_forward(sd, x)) <= 1e-5
    m.train()
    with torch.no_grad():
        got = m(x)
    ref = preresnet_forward(sd, x, training=True)
    assert rel_l2(got, ref) <= 1e-5
    for k in sd:
        if "running" in k:
            assert rel_l2(m.state_dict()[k], sd[k]) <= 1e-5, k
        if k.endswith("num_batches_tracked"):
            assert int(m.state_dict()[k]) == 1, k


def test_hooks_fire_with_the_right_operands_and_deepcopy(host_tensors):
    """downsample.0 reads the RAW block input (the output of layer1), not relu(bn1(.)) of it; conv2 reads relu(bn2(conv1(.)))."""
    from kdcc_amd.models import cifar_models
    m = cifar_models.preresnet(**SMALL["basic"]).eval()
    seeded_fill_(m, "preresnet.host.")
    names = ("layer1", "layer2", "layer2.0", "layer2.0.conv1", "layer2.0.conv2", "layer2.0.downsample.0", "layer2.1")
    seen = {}
    for name in names:
        m.get_submodule(name).register_forward_hook(lambda mod, i, o, name=name: seen.__setitem__(name, (i[0], o)))
    with torch.no_grad():
        m(seeded_input("preresnet.host.x", (2, 3, 32, 32)))
    assert set(seen) == set(names)
    blk = m.layer2[0]
    raw = seen["layer1"][1]
    assert torch.equal(seen["layer2"][0], raw) and torch.equal(seen["layer2.0"][0], raw)
    assert torch.equal(seen["layer2.0.downsample.0"][0], raw)
    with torch.no_grad():
        act = torch.relu(blk.bn1(raw))
        assert torch.equal(seen["layer2.0.conv1"][0], act) and not torch.equal(act, raw)
        assert torch.equal(seen["layer2.0.conv2"][0], torch.relu(blk.bn2(seen["layer2.0.conv1"][1])))
        h = torch.nn.functional.conv2d(seen["layer2.0.conv2"][0], blk.conv2.weight, padding=1)
    # (the residual add rides in the last conv: conv2's own output is already the block's)
    assert torch.equal(seen["layer2.0"][1], h + seen["layer2.0.downsample.0"][1])
    assert torch.equal(seen["layer2.0.conv2"][1], seen["layer2.0"][1])
    assert torch.equal(seen["layer2.1"][0], seen["layer2.0"][1]) and torch.equal(seen["layer2"][1], seen["layer2.1"][1])
    c = copy.deepcopy(m)
    assert c.layer1[0]._next[0] is c.layer1[1].bn1 and c.layer3[1]._next[0] is None
    with torch.no_grad():
        x = seeded_input("preresnet.host.x", (2, 3, 32, 32))
        assert torch.equal(c(x), m(x))


def test_host_tensors_are_refused_unless_allowed():
    from kdcc_amd import nn_hip
    from kdcc_amd._lib import KdccError
    from kdcc_amd.models import cifar_models
    nn_hip.allow_host_tensors(False)
    m = cifar_models.preresnet(**SMALL["basic"]).eval()
    with pytest.raises(KdccError), torch.no_grad():
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(KdccError):
        nn_hip.bn_relu_avgpool(m.bn, m.relu, torch.zeros(1, 64, 8, 8))
