#!/usr/bin/env python3
"""Generate tests/golden/wrn_keys.json and tests/golden/wrn.npz from the REFERENCE's own Wide-ResNet (CPU, fp32).

Runs only in the build container, like tools/make_golden.py, whose import recipe it reuses (it imports the reference, which
does not exist on the GPU box and must never travel).  Only data is written:
  * wrn_keys.json: state-dict key -> shape of wrn(depth=28, widen_factor=10, num_classes=100), and its parameter count;
  * wrn.npz, on a reduced WRN (depth 10, widen 4: 16 / 64 / 128 / 256 channels, stride-2 blocks with 1x1 shortcuts), seeded
    weights (tests/_seeded.py, prefix 'wrn.'), batch 8:
      - teacher eval logits; student (the same weights) train-mode logits, running statistics after that forward, the KLDiv(T=5)
        loss against the teacher and every parameter gradient (as 64 seeded projections, tests/_wrnref.py);
      - ClassificationTrainer._train_epoch(1) (3 SGD steps, lr 0.1) for a config-1-shaped plan (block3.layer.0 replaced in
        conv2, hinted, unfrozen) and a config-5-shaped plan (all of block2 unfrozen, block2.layer.0.conv2 replaced, block3
        hinted): the logged losses and the trainable parameters (projections).

    cd /path/to/reference && python3 /path/to/repo/tools/make_golden_wrn.py
"""
import copy
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                  # noqa: E402  (stubs, paths, DepthwiseStudent, save)

import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402

from models.cifar_models.wrn import wrn as ref_wrn         # noqa: E402
from _seeded import seeded_fill_, seeded_input             # noqa: E402
from _wrnref import project                                # noqa: E402

SMALL = dict(depth=10, widen_factor=4, num_classes=100)
PLANS = {
    "c1": {"hint": ["block3.layer.0"], "unfreeze": ["block3.layer.0"], "pruning_plan": ["block3.layer.0.conv2"]},
    "c5": {"hint": ["block3"], "unfreeze": ["block2"], "pruning_plan": ["block2.layer.0.conv2"]},
}


def wrn_config(plan, save_dir):
    cfgd = mg.trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
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


def g_keys():
    with torch.device("meta"):
        m = ref_wrn(depth=28, widen_factor=10, num_classes=100)
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    path = os.path.join(mg.OUT, "wrn_keys.json")
    with open(path, "w") as f:
        json.dump({"keys": keys, "num_params": sum(p.numel() for p in m.parameters())}, f, indent=0)
    print("wrote", path)


def g_small(out):
    import losses as ref_losses
    teacher = ref_wrn(**SMALL)
    seeded_fill_(teacher, "wrn.")
    teacher.eval()
    x = seeded_input("wrn.x", (8, 3, 32, 32))
    with torch.no_grad():
        out["teacher_logits"] = teacher(x)
    student = copy.deepcopy(teacher)
    student.train()
    s = student(x)
    loss = ref_losses.KLDivergenceLoss(temperature=5)(s, out["teacher_logits"])
    loss.backward()
    out["student_logits"] = s.detach()
    out["loss"] = loss.detach()
    for k, v in student.state_dict().items():
        if "running" in k:
            out["stat:" + k] = v
    for n, p in student.named_parameters():
        out["grad:" + n] = project(p.grad, n)


def g_trainer(out, plan):
    from parse_config import ConfigParser
    from trainer import ClassificationTrainer
    from utils import WeightScheduler
    from utils import optim as ref_optim
    import losses as ref_losses
    import models.metric as ref_metric
    config = ConfigParser(wrn_config(plan, tempfile.mkdtemp(prefix="kdgold_")), run_id=plan)
    teacher = ref_wrn(**SMALL)
    seeded_fill_(teacher, "wrn.")
    teacher.eval()
    model = mg.DepthwiseStudent(teacher, config)
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"wrn.student.{b['name']}.")
    model.replace = replace_and_seed
    crit = [config.init_obj(k, ref_losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(ref_metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", ref_optim, model.student.parameters())
    sched = config.init_obj("lr_scheduler", ref_optim.lr_scheduler, opt)
    batches = trainer_batches()
    tr = ClassificationTrainer(model, crit, metrics, opt, config, batches, None, sched, WeightScheduler(config["weight_scheduler"]))
    log = tr._train_epoch(1)
    for k, v in log.items():
        out[f"{plan}:log:{k}"] = np.float64(v)
    out[f"{plan}:trainable"] = np.array(sorted(n for n, p in model.student.named_parameters() if p.requires_grad))
    for n, p in model.student.named_parameters():
        if p.requires_grad:
            out[f"{plan}:param:{n}"] = project(p.data, n)


if __name__ == "__main__":
    torch.manual_seed(0)
    g_keys()
    out = {}
    g_small(out)
    for plan in PLANS:
        g_trainer(out, plan)
    mg.save("wrn", **out)
