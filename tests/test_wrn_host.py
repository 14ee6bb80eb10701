"""Wide-ResNet on the host: the checkpoint contract (keys / shapes / parameter count of the reference's WRN-28-10,
tests/golden/wrn_keys.json), every stored cfg/cifar100/wrn_28_10 config resolving and applying on the meta device, and a
host-plumbing forward against the stock-torch restatement in tests/_wrnref.py."""
import copy
import glob
import json
import os

import pytest
import torch

from _seeded import seeded_fill_, seeded_input
from _wrnref import rel_l2, wrn_forward

HERE = os.path.dirname(os.path.abspath(__file__))
CFG_DIR = os.path.join(HERE, "golden", "cfg", "cifar100", "wrn_28_10")
CONFIGS = sorted(glob.glob(os.path.join(CFG_DIR, "config*.json")))


def test_wrn28_10_keys_and_parameter_count_match_reference():
    from kdcc_amd.models import cifar_models
    with open(os.path.join(HERE, "golden", "wrn_keys.json")) as f:
        inv = json.load(f)
    with torch.device("meta"):
        m = cifar_models.wrn(depth=28, widen_factor=10, num_classes=100)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == inv["keys"]
    assert list(m.state_dict()) == list(inv["keys"])
    assert sum(p.numel() for p in m.parameters()) == inv["num_params"]


def test_all_seven_wrn_configs_are_stored():
    assert [os.path.basename(p) for p in CONFIGS] == [f"config{i}.json" for i in range(1, 8)]


@pytest.mark.parametrize("path", CONFIGS, ids=[os.path.basename(p) for p in CONFIGS])
def test_wrn_config_resolves_and_plan_applies(path, tmp_path):
    from kdcc_amd import ConfigParser, losses, nn_hip
    from kdcc_amd.models import cifar_models
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    from kdcc_amd import trainer as trainer_module
    from kdcc_amd.utils import optim as optim_module
    with open(path) as f:
        cfgd = json.load(f)
    cfgd["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfgd, run_id="w")
    with torch.device("meta"):
        teacher = config.init_obj("teacher", cifar_models)
        model = DepthwiseStudent(teacher, config)
    assert type(teacher).__name__ == "WideResNet"
    pr = cfgd["pruning"]
    for epoch in sorted({e["epoch"] for k in ("pruning_plan", "hint", "unfreeze") for e in pr[k]}):
        at = lambda k: [e for e in pr[k] if e["epoch"] == epoch]
        with torch.device("meta"):
            model.replace(at("pruning_plan"), **pr["args"])
        model.register_hint_layers([e["name"] for e in at("hint")])
        model.unfreeze([e["name"] for e in at("unfreeze")])
    for e in pr["pruning_plan"]:
        assert isinstance(model.get_block(e["name"], model.student), DepthwiseSeparableBlock)
    expect = set()
    for e in pr["unfreeze"]:
        expect |= {f"{e['name']}.{n}" for n, _ in model.get_block(e["name"], model.student).named_parameters()}
    assert {n for n, p in model.student.named_parameters() if p.requires_grad} == expect
    assert len(model._student_hook_handlers) == len({e["name"] for e in pr["hint"]})
    for m in model.teacher.modules():
        if isinstance(m, torch.nn.Conv2d):
            assert type(m) is nn_hip.Conv2dNHWC
        if isinstance(m, torch.nn.BatchNorm2d):
            assert type(m) is nn_hip.BatchNorm2dNHWC
    opt = config.init_obj("optimizer", optim_module, [p for p in model.student.parameters() if p.requires_grad])
    assert type(opt).__name__ == "SGD"
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    assert type(sched).__name__ == "MultiStepLR"
    assert hasattr(trainer_module, cfgd["trainer"]["name"])
    for k in ("supervised_loss", "kd_loss", "hint_loss"):
        config.init_obj(k, losses)


def test_wrn_host_forward_matches_stock_torch():
    from kdcc_amd import nn_hip
    from kdcc_amd.models import cifar_models
    nn_hip.allow_host_tensors(True)
    try:
        m = cifar_models.wrn(depth=10, widen_factor=2, num_classes=10)
        seeded_fill_(m, "wrn.host.")
        x = seeded_input("wrn.host.x", (2, 3, 32, 32))
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            assert rel_l2(m(x), wrn_forward(sd, x, depth=10)) <= 1e-5
        m.train()
        with torch.no_grad():
            got = m(x)
        ref = wrn_forward(sd, x, depth=10, training=True)
        assert rel_l2(got, ref) <= 1e-5
        for k in sd:
            if "running" in k:
                assert rel_l2(m.state_dict()[k], sd[k]) <= 1e-5, k
    finally:
        nn_hip.allow_host_tensors(False)


def test_wrn_block_quirk_and_children_called_as_modules():
    """Where width changes, conv1 and the shortcut both read relu(bn1(x)); hooks on a block and on its convs fire."""
    from kdcc_amd import nn_hip
    from kdcc_amd.models import cifar_models
    nn_hip.allow_host_tensors(True)
    try:
        m = cifar_models.wrn(depth=10, widen_factor=2, num_classes=10).eval()
        blk = m.block2.layer[0]
        assert blk.convShortcut is not None and m.block1.layer[0].convShortcut is not None
        seen = {}
        for name in ("block2.layer.0", "block2.layer.0.conv1", "block2.layer.0.convShortcut", "block2.layer.0.conv2", "block3"):
            mod = m.get_submodule(name)
            mod.register_forward_hook(lambda mod, i, o, name=name: seen.__setitem__(name, (i[0], o)))
        with torch.no_grad():
            m(seeded_input("wrn.host.x", (2, 3, 32, 32)))
        assert torch.equal(seen["block2.layer.0.conv1"][0], seen["block2.layer.0.convShortcut"][0])
        assert set(seen) == {"block2.layer.0", "block2.layer.0.conv1", "block2.layer.0.convShortcut", "block2.layer.0.conv2", "block3"}
        with pytest.raises(NotImplementedError):
            cifar_models.wrn(depth=10, widen_factor=1, num_classes=10, dropRate=0.3).train()(torch.zeros(1, 3, 32, 32))
        copy.deepcopy(m)
    finally:
        nn_hip.allow_host_tensors(False)
