"""CPU: the reference's four ensemble.json configs resolve and their plans apply on the meta device; the float64 restatement of
kd_kldiv_multi / kd_softmax_mean (tests/_ensemble_ref.py) reproduces the reference's recorded values (tests/golden/ensemble.npz,
tools/make_golden_ensemble.py) -- the GPU tests lean on it; and EnsembleTrainer's host-side logic (resume_ensemble, the reset()
quirk, its refusals) in the explicit host plumbing mode."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import _ensemble_ref as R
from _ensemble_util import MEMBER_PLANS, PLANS, build_trainer, crit_case, ensemble_config, member_checkpoint, seeded_teacher
from _seeded import seeded_value
from _wrnref import project, rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = sorted(glob.glob(os.path.join(HERE, "golden", "cfg", "cifar10*", "*", "ensemble.json")))


@pytest.fixture(scope="module")
def ens():
    return np.load(os.path.join(HERE, "golden", "ensemble.npz"), allow_pickle=False)


def test_all_four_ensemble_configs_are_stored():
    rel = [os.path.relpath(p, os.path.join(HERE, "golden", "cfg")) for p in CONFIGS]
    assert rel == ["cifar10/resnet20/ensemble.json", "cifar10/resnet44/ensemble.json", "cifar10/resnet56/ensemble.json",
                   "cifar100/wrn_28_10/ensemble.json"]


@pytest.mark.parametrize("path", CONFIGS, ids=[p.split(os.sep)[-2] for p in CONFIGS])
def test_ensemble_config_resolves_and_plan_applies(path, tmp_path):
    from kdcc_amd import ConfigParser, losses
    from kdcc_amd import trainer as trainer_module
    from kdcc_amd.models import cifar_models
    from kdcc_amd.models.students import DepthwiseStudent, EnsembleStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    from kdcc_amd.utils import optim as optim_module
    with open(path) as f:
        cfgd = json.load(f)
    cfgd["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfgd, run_id="e")
    assert cfgd["trainer"]["name"] == "EnsembleTrainer" and len(cfgd["trainer"]["resume_paths"]) >= 1
    assert issubclass(getattr(trainer_module, cfgd["trainer"]["name"]), trainer_module.ClassificationTrainer)
    assert hasattr(cifar_models, cfgd["teacher"]["type"])
    with torch.device("meta"):
        teacher = config.init_obj("teacher", cifar_models)
        model = EnsembleStudent(teacher, config)
    assert isinstance(model, DepthwiseStudent) and len(model.studdents) == 0 and not model.fused
    pr = cfgd["pruning"]
    with torch.device("meta"):
        model.replace(pr["pruning_plan"], **pr["args"])       # (the WRN file names block2.layer.1.conv2 twice)
    model.register_hint_layers([e["name"] for e in pr["hint"]])
    model.unfreeze([e["name"] for e in pr["unfreeze"]])
    for e in pr["pruning_plan"]:
        assert isinstance(model.get_block(e["name"], model.student), DepthwiseSeparableBlock)
    model.reset()
    assert not any(isinstance(m, DepthwiseSeparableBlock) for m in model.student.modules()) and model.replaced_block_names == []
    opt = config.init_obj("optimizer", optim_module, [torch.nn.Parameter(torch.zeros(1))])
    assert type(opt).__name__ == cfgd["optimizer"]["type"]
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    assert type(sched).__name__ == cfgd["lr_scheduler"]["type"]
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    assert type(crit[0]) is losses.CrossEntropyLoss2d and type(crit[1]) is losses.KLDivergenceLoss
    assert crit[1].temperature == cfgd["kd_loss"]["args"]["temperature"]


@pytest.mark.parametrize("tag", ["crit2d", "crit4d"])
@pytest.mark.parametrize("T", [1, 5])
def test_restatement_reproduces_the_reference_criterion(ens, tag, T):
    g = ens
    s, ts, labels, w = crit_case(g, tag)
    if tag == "crit4d":
        assert (labels == 255).any()
    r = R.kldiv_multi(s, ts, w, T, labels, 255)
    key = f"{tag}_T{T}"
    np.testing.assert_allclose([e.item() for e in r["kd_each"]], g[f"{key}.kd_each"], rtol=1e-4, atol=1e-7)
    for k in ("kd", "sup"):
        np.testing.assert_allclose(r[k].item(), g[f"{key}.{k}"], rtol=1e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(r["total"].item(), g[f"{key}.loss"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(r["grad"].numpy(), g[f"{key}.grad"], rtol=1e-3, atol=1e-7)
    # the loss is NOT the KL to the averaged distribution (only the gradient is linear in the targets)
    mean_t = R.softmax_mean(ts, w, T)
    kl_to_mean = T * T / (s.numel() // s.shape[1]) * (torch.xlogy(mean_t, mean_t) - mean_t * torch.log_softmax(s.double() / T, 1)).sum()
    assert abs(kl_to_mean.item() - r["kd"].item()) > 1e-3 * abs(r["kd"].item())


def test_restatement_without_labels_and_with_all_ignored(ens):
    s, ts, labels, w = crit_case(ens, "crit4d")
    a = R.kldiv_multi(s, ts, w, 5, None)
    b = R.kldiv_multi(s, ts, w, 5, torch.full_like(labels, 255), 255)
    assert a["sup"].item() == 0.0 and b["sup"].item() == 0.0 and torch.equal(a["grad"], b["grad"])
    assert torch.allclose(R.softmax_mean(ts, w, 1.0).sum(1), torch.ones(2, 8, 16, dtype=torch.float64), atol=1e-12)


@pytest.fixture
def host_mode():
    from kdcc_amd import nn_hip
    nn_hip.allow_host_tensors(True)
    try:
        yield
    finally:
        nn_hip.allow_host_tensors(False)


def test_resume_ensemble_members_quirk_and_refusals(ens, tmp_path, host_mode):
    from kdcc_amd import ConfigParser
    from kdcc_amd.models import DeepWV3Plus
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    from kdcc_amd.trainer import EnsembleTrainer
    paths = [member_checkpoint(i, plan, str(tmp_path)) for i, plan in enumerate(MEMBER_PLANS)]
    tr = build_trainer(ensemble_config(str(tmp_path), paths, n_gpu=0))
    assert len(tr.models) == int(ens["n_members"]) == 2
    for member, plan in zip(tr.models, MEMBER_PLANS):
        dw = sorted(n for n, m in member.named_modules() if isinstance(m, DepthwiseSeparableBlock))
        assert dw == sorted(PLANS[plan]["pruning_plan"])
    tr.prepare_models(1)
    for member in tr.models:
        assert not member.training and not any(p.requires_grad for p in member.parameters())
    assert not any(p.requires_grad for p in tr.model.teacher.parameters()) and not tr.model.teacher.training
    assert all(p.requires_grad for p in tr.model.student.parameters()) and tr.model.student.training
    # the student to be trained: no replaced block left, and the LAST checkpoint's weights where nothing was replaced
    student = tr.model.student
    assert not any(isinstance(m, DepthwiseSeparableBlock) for m in student.modules()) and tr.model.replaced_block_names == []
    w = student.block1.layer[0].conv1.weight.detach()
    assert torch.equal(w, seeded_value("ens.m1.block1.layer.0.conv1.weight", w))
    assert not torch.equal(w, seeded_value("wrn.block1.layer.0.conv1.weight", w))
    assert rel_l2(project(w, "block1.layer.0.conv1.weight"), ens["quirk:block1.layer.0.conv1.weight"]) <= 1e-6
    # ... while a replaced block is the teacher's again, and the teacher took the checkpoint's (identical) teacher.* entries
    w2 = student.block2.layer[0].conv2.weight.detach()
    assert torch.equal(w2, seeded_value("wrn.block2.layer.0.conv2.weight", w2))
    assert torch.equal(tr.model.teacher.fc.weight, seeded_value("wrn.fc.weight", w2.new_empty(tr.model.teacher.fc.weight.shape)))
    # (the members' cheap blocks have no host path: ensemble_predict and the epoch are held to the golden in test_ensemble_gpu.py)

    with pytest.raises(ValueError, match="resume_paths"):
        build_trainer(ensemble_config(str(tmp_path), None, n_gpu=0), run_id="nopaths")
    cfgd = ensemble_config(str(tmp_path), paths, n_gpu=0)
    with torch.device("meta"):
        fused = DepthwiseStudent(DeepWV3Plus(num_classes=19), None)
    assert fused.fused
    with pytest.raises(NotImplementedError, match="classification"):
        EnsembleTrainer(fused, [], [], None, ConfigParser(cfgd, run_id="fused"), [])


def test_ops_refuse_host_tensors():
    from kdcc_amd import ops
    from kdcc_amd._lib import KdccError
    with pytest.raises(KdccError):
        ops.kldiv_multi(torch.zeros(2, 4), [torch.zeros(2, 4)], [1.0], 1.0)
    with pytest.raises(KdccError):
        ops.softmax_mean([torch.zeros(2, 4)], [1.0], 1.0)
