"""Shared by the EnsembleTrainer tests: the reduced WRN, the two seeded member checkpoints and the trainer around them, built with this
package exactly as tools/make_golden_ensemble.py builds them with the reference."""
import os

import torch

from _netutil import trainer_config
from _seeded import seeded_fill_, seeded_input

SMALL = dict(depth=10, widen_factor=4, num_classes=100)
PLANS = {
    "c1": {"hint": ["block3.layer.0"], "unfreeze": ["block3.layer.0"], "pruning_plan": ["block3.layer.0.conv2"]},
    "c5": {"hint": ["block3"], "unfreeze": ["block2"], "pruning_plan": ["block2.layer.0.conv2"]},
}
MEMBER_PLANS = ("c1", "c5")
WEIGHTS = (1.0, 2.0, 0.5)


def wrn_config(plan, save_dir, n_gpu=1):
    cfgd = trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir, n_gpu=n_gpu)
    cfgd.update(name="golden_wrn", teacher={"type": "wrn", "args": dict(SMALL)}, optimizer={"type": "SGD", "args": {"lr": 0.1}},
                kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
                hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}},
                metrics=["accuracy", "top_k_acc"],
                lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}})
    cfgd["trainer"]["name"] = "ClassificationTrainer"
    cfgd["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3},
                       **{k: [{"name": n, "epoch": 1} for n in v] for k, v in PLANS[plan].items()}}
    return cfgd


def trainer_batches():
    return [(seeded_input(f"wrn.tr.x{i}", (8, 3, 32, 32)),
             torch.randint(0, 100, (8,), generator=torch.Generator().manual_seed(300 + i))) for i in range(3)]


def seeded_teacher():
    from kdcc_amd.models import cifar_models
    teacher = cifar_models.wrn(**SMALL)
    seeded_fill_(teacher, "wrn.")
    return teacher.eval()


def member_checkpoint(index, plan, save_dir):
    from kdcc_amd.models.students import DepthwiseStudent
    cfgd = wrn_config(plan, save_dir)
    model = DepthwiseStudent(seeded_teacher(), cfgd)
    model.replace(cfgd["pruning"]["pruning_plan"], **cfgd["pruning"]["args"])
    seeded_fill_(model.student, f"ens.m{index}.")
    path = os.path.join(save_dir, f"member{index}.pth")
    torch.save({"config": cfgd, "epoch": 1, "state_dict": model.state_dict(), "monitor_best": 0}, path)
    return path


def ensemble_config(save_dir, paths, n_gpu=1):
    cfgd = wrn_config("c5", save_dir, n_gpu=n_gpu)
    cfgd["name"] = "golden_ensemble"
    cfgd["trainer"]["name"] = "EnsembleTrainer"
    if paths is not None:
        cfgd["trainer"]["resume_paths"] = list(paths)
    return cfgd


def build_trainer(cfgd, run_id="ens", teacher=None, batches=None, device=None):
    from kdcc_amd import ConfigParser, losses
    from kdcc_amd.models import metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer import EnsembleTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    config = ConfigParser(cfgd, run_id=run_id)
    teacher = seeded_teacher() if teacher is None else teacher
    if device is not None:
        teacher = teacher.to(device)
    model = DepthwiseStudent(teacher, config)
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    batches = trainer_batches() if batches is None else batches
    return EnsembleTrainer(model, crit, metrics, opt, config, batches, batches, sched, WeightScheduler(config["weight_scheduler"]))


def crit_case(g, tag, device="cpu"):
    s = torch.from_numpy(g[f"{tag}.s"]).to(device)
    ts = [torch.from_numpy(g[f"{tag}.t{k}"]).to(device) for k in range(len(WEIGHTS))]
    return s, ts, torch.from_numpy(g[f"{tag}.labels"]).to(device), [float(w) for w in g[f"{tag}.w"]]
