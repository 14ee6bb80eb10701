"""CPU: the layer-compressibility analysis at the plan level.  RandomMask2d draws what the reference draws from numpy's global
state; both cfg/cityscapes/analysis_compressible configs (verbatim copies under tests/golden/cfg/) resolve, every one of their 20
layer names replaces / registers / is a masked engine site / resets on the meta device; AnalysisTrainer.train() walks layers x
learning rates x (epochs - 1) epochs the way the reference does (trainer/analysis_trainer.py:13-39)."""
import glob
import json
import os
import types

import numpy as np
import pytest
import torch
from torch import nn

import kdcc_amd  # noqa: F401
from kdcc_amd import models

CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg", "cityscapes", "analysis_compressible")
CONFIGS = sorted(glob.glob(os.path.join(CFG_DIR, "*.json")))


@pytest.mark.parametrize("C,droprate,seed", [(512, 0.85, 0), (256, 0.85, 7), (2048, 0.85, 3), (64, 0.9, 11), (10, 0.25, 5)])
def test_random_mask_is_the_reference_draw(C, droprate, seed):
    from kdcc_amd.models.students import RandomMask2d
    np.random.seed(seed)
    m = RandomMask2d(C, droprate)
    # the reference's draw, restated (models/students/transform_blocks/mask.py:23-26)
    np.random.seed(seed)
    ref = np.ones((1, C, 1, 1), dtype=np.float32)
    ref[0][np.random.choice(C, int(C * droprate), False)] = 0
    assert m.mask.dtype == torch.float32 and tuple(m.mask.shape) == (1, C, 1, 1)
    assert np.array_equal(m.mask.numpy(), ref)
    assert int((m.mask == 0).sum()) == int(C * droprate)
    assert "mask" not in m.state_dict() and list(m.state_dict()) == [] and list(m.parameters()) == []
    assert m.keep.dtype == torch.int64 and m.keep.tolist() == np.flatnonzero(ref.reshape(-1)).tolist()
    assert m.keep.tolist() == sorted(m.keep.tolist()) and m.keep.numel() == C - int(C * droprate)
    x = torch.randn(2, C, 3, 4)
    assert torch.equal(m(x), torch.from_numpy(ref) * x)                 # the non-fused path
    assert m.to("meta").mask.device.type == "meta" and m.keep.device.type == "cpu"


def test_kept_counts_at_the_config_droprate():
    from kdcc_amd.models.students import RandomMask2d
    assert [RandomMask2d(c, 0.85).keep.numel() for c in (512, 1024, 2048, 256)] == [77, 154, 308, 39]


def test_the_stored_analysis_configs_are_all_there():
    assert [os.path.basename(p) for p in CONFIGS] == ["deeplabwv3p.json", "gscnn.json"]


@pytest.mark.parametrize("path", CONFIGS, ids=[os.path.basename(p) for p in CONFIGS])
def test_analysis_config_resolves_and_every_layer_applies(path):
    from kdcc_amd.engine import EngineError, StudentEngine, _Site
    from kdcc_amd.models.students import AnalysisStudent, RandomMask2d
    cfg = json.load(open(path))
    assert cfg["teacher"]["type"] == {"deeplabwv3p.json": "DeepWV3Plus", "gscnn.json": "GSCNN"}[os.path.basename(path)]
    for key in ("supervised_loss", "kd_loss", "hint_loss"):
        assert hasattr(kdcc_amd.losses, cfg[key]["type"]), cfg[key]["type"]
    assert cfg["supervised_loss"]["type"] == "CrossEntropyLoss2d" and cfg["kd_loss"]["type"] == cfg["hint_loss"]["type"] == "MSELoss"
    assert hasattr(kdcc_amd.utils.optim, cfg["optimizer"]["type"])
    assert hasattr(kdcc_amd.utils.optim.lr_scheduler, cfg["lr_scheduler"]["type"])
    assert cfg["trainer"]["name"] == "AnalysisTrainer"
    assert getattr(kdcc_amd.trainer, cfg["trainer"]["name"]) is kdcc_amd.trainer.AnalysisTrainer
    layers = cfg["layer_compressible"]
    assert len(layers) == 20 and all(len(l["lrs"]) == 5 and l["args"] == {"droprate": 0.85} for l in layers)
    with torch.device("meta"):
        teacher = getattr(models, cfg["teacher"]["type"])(**cfg["teacher"]["args"])
        model = AnalysisStudent(teacher, None)
    assert model.fused
    teacher_keys = list(model.teacher.state_dict())
    for layer in layers:
        name = layer["layer_name"]
        with torch.device("meta"):
            model.replace([name], **layer["args"])
        model.register_hint_layers([name])                              # validated against the fused graph
        assert model.hint_block_names == [name] and model.replaced_block_names == [name]
        blk = model.get_block(name, model.student)
        tblk = model.get_block(name, model.teacher)
        assert isinstance(blk, nn.Sequential) and isinstance(blk[1], RandomMask2d) and blk[2].bias is None
        assert blk[2].kernel_size == (1, 1) and blk[2].in_channels == blk[2].out_channels == tblk.out_channels
        assert blk[1].keep.numel() == tblk.out_channels - int(tblk.out_channels * 0.85)
        site = _Site(name, blk)
        assert site.masked and not site.cheap and site.trainable
        assert (site.cin, site.cout, site.k, site.dil, site.stride) == (tblk.in_channels, tblk.out_channels, tblk.kernel_size[0],
                                                                        tblk.dilation[0], tblk.stride[0])
        trainable = [n for n, p in model.student.named_parameters() if p.requires_grad]
        assert trainable == [name + ".2.weight"]
        eng = StudentEngine(model.student, torch.bfloat16)
        eng.check_hint_names([name])
        order = eng.grad_production_order()
        assert len(order) == 1 and order[0] is blk[2].weight
        with torch.device("meta"):
            model.reset()
        assert list(model.student.state_dict()) == teacher_keys and model.replaced_block_names == [] and model.hint_block_names == []
        assert isinstance(model.get_block(name, model.student), nn.Conv2d)
    # a trainable conv in front of the mask is not the probe the engine implements
    with torch.device("meta"):
        model.replace(["mod4.block2.convs.conv2"], droprate=0.85)
    model.get_block("mod4.block2.convs.conv2", model.student)[0].weight.requires_grad = True
    with pytest.raises(EngineError):
        _Site("mod4.block2.convs.conv2", model.get_block("mod4.block2.convs.conv2", model.student))


def test_analysis_student_replace_takes_strings_and_a_droprate():
    from kdcc_amd.models.students import AnalysisStudent, DepthwiseStudent
    assert issubclass(AnalysisStudent, DepthwiseStudent)
    with torch.device("meta"):
        model = AnalysisStudent(models.DeepWV3Plus(num_classes=19), None)
        with pytest.raises(KeyError):
            model.replace(["mod4.block2.convs.conv2"])                  # droprate= is required, as in the reference


class _StubModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.student = nn.Linear(2, 2)
        self.calls = []

    def replace(self, names, **kw):
        self.calls.append(("replace", tuple(names), kw))

    def register_hint_layers(self, names):
        self.calls.append(("hint", tuple(names)))

    def reset(self):
        self.calls.append(("reset",))

    def dump_trainable_params(self):
        return ""

    def dump_student_teacher_blocks_info(self):
        return ""


def test_analysis_trainer_train_walks_layers_lrs_epochs(tmp_path):
    """(epochs - 1) x len(lrs) x len(layers) epochs; per learning rate: replace, hint registration, scheduler reset, a NEW optimizer
    whose every param group carries that learning rate, and a reset afterwards."""
    from _netutil import trainer_config
    from kdcc_amd import ConfigParser
    from kdcc_amd.trainer import AnalysisTrainer, LayerwiseTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    assert issubclass(AnalysisTrainer, LayerwiseTrainer)
    cfg = trainer_config([], lr=0.005, len_epoch=1, save_dir=str(tmp_path), n_gpu=0)
    cfg["trainer"].update(name="AnalysisTrainer", epochs=3)
    layers = [{"layer_name": "mod4.block2.convs.conv2", "lrs": [0.01, 0.001], "args": {"droprate": 0.85}},
              {"layer_name": "aspp.features.1.0", "lrs": [0.005, 0.0005, 0.0001], "args": {"droprate": 0.5}}]
    cfg["layer_compressible"] = layers
    config = ConfigParser(cfg, run_id="a")
    model = _StubModel()
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    tr = AnalysisTrainer(model, [nn.Identity(), nn.Identity(), nn.Identity()], [], opt, config, [], None, sched,
                         WeightScheduler(config["weight_scheduler"]))
    seen, resets = [], []
    tr.reset_scheduler = lambda: resets.append(1)

    def fake_epoch(epoch, **kw):
        assert tr.optimizer is not opt and all(g["lr"] == kw["lr"] for g in tr.optimizer.param_groups)
        seen.append((epoch, kw["lr"], kw["layer_name"], id(tr.optimizer)))
    tr._train_epoch = fake_epoch
    tr.train()
    want = [(e, lr, l["layer_name"]) for l in layers for lr in l["lrs"] for e in range(1, 3)]
    assert [s[:3] for s in seen] == want and len(seen) == (3 - 1) * 5
    assert len({s[3] for s in seen}) >= 2 and len(resets) == 5          # one optimizer / scheduler reset per learning rate
    flat = [c for c in model.calls]
    per_lr = [("replace", ("mod4.block2.convs.conv2",), {"droprate": 0.85}), ("hint", ("mod4.block2.convs.conv2",)), ("reset",)]
    assert flat[:3] == per_lr and flat[3:6] == per_lr
    assert flat[6] == ("replace", ("aspp.features.1.0",), {"droprate": 0.5}) and len(flat) == 15


def test_metric_tracker_takes_a_ready_confusion_matrix():
    from kdcc_amd.utils import CityscapesMetricTracker
    g = torch.Generator().manual_seed(0)
    logits, labels = torch.randn(2, 19, 8, 8, generator=g), torch.randint(0, 19, (2, 8, 8), generator=g)
    a, b = CityscapesMetricTracker(), CityscapesMetricTracker()
    a.update(logits, labels); a.update(logits, labels)
    b.add_confusion(a.conf // 2); b.add_confusion(a.conf // 2)
    assert torch.equal(a.conf, b.conf) and a.get_iou() == b.get_iou()
    with pytest.raises(ValueError):
        b.add_confusion(torch.zeros(3, 3, dtype=torch.int64))
