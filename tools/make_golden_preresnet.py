#!/usr/bin/env python3
"""Generate tests/golden/preresnet_keys.json and tests/golden/preresnet.npz from the REFERENCE's own PreResNet (CPU, fp32).

Runs only in the build container, like tools/make_golden_wrn.py, whose recipe it follows (it imports the reference, which does
not exist on the GPU box and must never travel).  Only data is written:
  * preresnet_keys.json: state-dict key -> shape and the parameter count of preresnet(depth=110, num_classes=100) ("basic") and of
    preresnet(depth=164, num_classes=100, block_name='Bottleneck') ("bottleneck");
  * preresnet.npz, on two reduced nets with an identity block behind a downsample block in every layer -- depth 14 BasicBlock
    ("basic:") and depth 20 Bottleneck ("bottleneck:") --, seeded weights (tests/_seeded.py, prefix 'preresnet.'), batch 8:
      - teacher eval logits; student (the same weights) train-mode logits, running statistics after that forward, the KLDiv(T=5)
        loss against the teacher and every parameter gradient (as 64 seeded projections, tests/_wrnref.py);
      - for the BasicBlock net, ClassificationTrainer._train_epoch(1) (3 SGD steps, lr 0.1) for a plan of the WRN goldens' shape
        (layer3.1.conv2 replaced, layer3.1 hinted and unfrozen): the logged losses and the trainable parameters (projections).

    cd /path/to/reference && python3 /path/to/repo/tools/make_golden_preresnet.py
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

from models.cifar_models.preresnet import preresnet as ref_preresnet   # noqa: E402
from _seeded import seeded_fill_, seeded_input             # noqa: E402
from _wrnref import project                                # noqa: E402

FULL = {"basic": dict(depth=110, num_classes=100), "bottleneck": dict(depth=164, num_classes=100, block_name="Bottleneck")}
SMALL = {"basic": dict(depth=14, num_classes=100), "bottleneck": dict(depth=20, num_classes=100, block_name="Bottleneck")}
PLAN = {"hint": ["layer3.1"], "unfreeze": ["layer3.1"], "pruning_plan": ["layer3.1.conv2"]}


def preresnet_config(save_dir):
    cfgd = mg.trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
    cfgd.update(name="golden_preresnet", teacher={"type": "preresnet", "args": dict(SMALL["basic"])},
                optimizer={"type": "SGD", "args": {"lr": 0.1}},
                kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
                hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}},
                metrics=["accuracy", "top_k_acc"],
                lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}})
    cfgd["trainer"]["name"] = "ClassificationTrainer"
    cfgd["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3},
                       **{k: [{"name": n, "epoch": 1} for n in v] for k, v in PLAN.items()}}
    return cfgd


def trainer_batches():
    return [(seeded_input(f"preresnet.tr.x{i}", (8, 3, 32, 32)),
             torch.randint(0, 100, (8,), generator=torch.Generator().manual_seed(300 + i))) for i in range(3)]


def g_keys():
    inv = {}
    for kind, args in FULL.items():
        with torch.device("meta"):
            m = ref_preresnet(**args)
        inv[kind] = {"keys": {k: list(v.shape) for k, v in m.state_dict().items()},
                     "num_params": sum(p.numel() for p in m.parameters())}
    path = os.path.join(mg.OUT, "preresnet_keys.json")
    with open(path, "w") as f:
        json.dump(inv, f, indent=0)
    print("wrote", path, {k: (len(v["keys"]), v["num_params"]) for k, v in inv.items()})


def g_small(out, kind):
    import losses as ref_losses
    teacher = ref_preresnet(**SMALL[kind])
    seeded_fill_(teacher, "preresnet.")
    teacher.eval()
    x = seeded_input("preresnet.x", (8, 3, 32, 32))
    with torch.no_grad():
        out[f"{kind}:teacher_logits"] = teacher(x)
    student = copy.deepcopy(teacher)
    student.train()
    s = student(x)
    loss = ref_losses.KLDivergenceLoss(temperature=5)(s, out[f"{kind}:teacher_logits"])
    loss.backward()
    out[f"{kind}:student_logits"] = s.detach()
    out[f"{kind}:loss"] = loss.detach()
    for k, v in student.state_dict().items():
        if "running" in k:
            out[f"{kind}:stat:" + k] = v
    for n, p in student.named_parameters():
        out[f"{kind}:grad:" + n] = project(p.grad, n)


def g_trainer(out):
    from parse_config import ConfigParser
    from trainer import ClassificationTrainer
    from utils import WeightScheduler
    from utils import optim as ref_optim
    import losses as ref_losses
    import models.metric as ref_metric
    config = ConfigParser(preresnet_config(tempfile.mkdtemp(prefix="kdgold_")), run_id="plan")
    teacher = ref_preresnet(**SMALL["basic"])
    seeded_fill_(teacher, "preresnet.")
    teacher.eval()
    model = mg.DepthwiseStudent(teacher, config)
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"preresnet.student.{b['name']}.")
    model.replace = replace_and_seed
    crit = [config.init_obj(k, ref_losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(ref_metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", ref_optim, model.student.parameters())
    sched = config.init_obj("lr_scheduler", ref_optim.lr_scheduler, opt)
    tr = ClassificationTrainer(model, crit, metrics, opt, config, trainer_batches(), None, sched,
                               WeightScheduler(config["weight_scheduler"]))
    log = tr._train_epoch(1)
    for k, v in log.items():
        out[f"plan:log:{k}"] = np.float64(v)
    out["plan:trainable"] = np.array(sorted(n for n, p in model.student.named_parameters() if p.requires_grad))
    for n, p in model.student.named_parameters():
        if p.requires_grad:
            out[f"plan:param:{n}"] = project(p.data, n)


if __name__ == "__main__":
    torch.manual_seed(0)
    g_keys()
    out = {}
    for kind in SMALL:
        g_small(out, kind)
    g_trainer(out)
    mg.save("preresnet", **out)
