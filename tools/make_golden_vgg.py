#!/usr/bin/env python3
"""Generate tests/golden/vgg_keys.json and tests/golden/vgg.npz from the REFERENCE's own CIFAR VGG (CPU, fp32).

Runs only in the build container, like tools/make_golden_preresnet.py, whose recipe it follows (it imports the reference, which
does not exist on the GPU box and must never travel).  Only data is written:
  * vgg_keys.json: state-dict key -> shape and the parameter count of vgg16_bn(num_classes=10) ("vgg16_bn") and of
    vgg19(num_classes=100) ("vgg19");
  * vgg.npz, on two reduced nets -- VGG(make_layers([16, 'M', 32, 'M', 64, 64, 'M', 64, 'M', 512, 'M'], batch_norm), 100) with
    BatchNorm ("bn:") and without ("plain:") --, seeded weights (tests/_seeded.py, prefix 'vgg.'), batch 8:
      - teacher eval logits; student train-mode logits (the same weights with BatchNorm, whose batch statistics make it differ; the
        weights of prefix 'vgg.student.' without), running statistics after that forward, the KLDiv(T=5) loss against the teacher
        and every parameter gradient (as 64 seeded projections, tests/_wrnref.py);
      - a host-plumbing forward of the BatchNorm net: eval logits of batch 2 under the prefix 'vgg.host.' ("host:logits");
      - for the BatchNorm net, ClassificationTrainer._train_epoch(1) (3 SGD steps, lr 0.1) for a plan of the WRN goldens' shape
        (features.11, the second 64-channel conv, replaced, hinted and unfrozen): the logged losses and the trainable parameters
        (projections).  The reference's DepthwiseStudent.replace hands nn.Conv2d the teacher conv's bias TENSOR as its `bias` flag,
        which torch refuses for a vector of more than one element; what it means is "biased", and replace() below says so.

    cd /path/to/reference && python3 /path/to/repo/tools/make_golden_vgg.py
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

from models.cifar_models import vgg as ref_vgg             # noqa: E402
from _seeded import seeded_fill_, seeded_input             # noqa: E402
from _wrnref import project                                # noqa: E402

FULL = {"vgg16_bn": dict(num_classes=10), "vgg19": dict(num_classes=100)}
SMALL_CFG = [16, "M", 32, "M", 64, 64, "M", 64, "M", 512, "M"]
SMALL = {"bn": True, "plain": False}
PLAN = {"hint": ["features.11"], "unfreeze": ["features.11"], "pruning_plan": ["features.11"]}


def small(kind):
    return ref_vgg.VGG(ref_vgg.make_layers(SMALL_CFG, batch_norm=SMALL[kind]), num_classes=100)


def vgg_config(save_dir):
    cfgd = mg.trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
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


def trainer_batches():
    return [(seeded_input(f"vgg.tr.x{i}", (8, 3, 32, 32)),
             torch.randint(0, 100, (8,), generator=torch.Generator().manual_seed(300 + i))) for i in range(3)]


def g_keys():
    inv = {}
    for kind, args in FULL.items():
        with torch.device("meta"):
            m = getattr(ref_vgg, kind)(**args)
        inv[kind] = {"keys": {k: list(v.shape) for k, v in m.state_dict().items()},
                     "num_params": sum(p.numel() for p in m.parameters())}
    path = os.path.join(mg.OUT, "vgg_keys.json")
    with open(path, "w") as f:
        json.dump(inv, f, indent=0)
    print("wrote", path, {k: (len(v["keys"]), v["num_params"]) for k, v in inv.items()})


def g_small(out, kind):
    import losses as ref_losses
    teacher = small(kind)
    seeded_fill_(teacher, "vgg.")
    teacher.eval()
    x = seeded_input("vgg.x", (8, 3, 32, 32))
    with torch.no_grad():
        out[f"{kind}:teacher_logits"] = teacher(x)
    student = copy.deepcopy(teacher)
    if not SMALL[kind]:     # (without BatchNorm train mode is eval mode: a copy would give a zero loss and no gradient to compare)
        seeded_fill_(student, "vgg.student.")
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


def g_host(out):
    m = small("bn")
    seeded_fill_(m, "vgg.host.")
    m.eval()
    with torch.no_grad():
        out["host:logits"] = m(seeded_input("vgg.host.x", (2, 3, 32, 32)))


def g_trainer(out):
    from parse_config import ConfigParser
    from trainer import ClassificationTrainer
    from utils import WeightScheduler
    from utils import optim as ref_optim
    import losses as ref_losses
    import models.metric as ref_metric
    config = ConfigParser(vgg_config(tempfile.mkdtemp(prefix="kdgold_")), run_id="plan")
    teacher = small("bn")
    seeded_fill_(teacher, "vgg.")
    teacher.eval()
    model = mg.DepthwiseStudent(teacher, config)
    orig_replace = model.replace
    import models.students.depthwise_student as ref_ds
    ref_block = ref_ds.DepthwiseSeparableBlock

    def replace_and_seed(blocks, **kw):
        ref_ds.DepthwiseSeparableBlock = lambda *a, bias=None, **k: ref_block(*a, bias=bias is not None and bias is not False, **k)
        try:
            orig_replace(blocks, **kw)
        finally:
            ref_ds.DepthwiseSeparableBlock = ref_block
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"vgg.student.{b['name']}.")
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
    g_host(out)
    g_trainer(out)
    mg.save("vgg", **out)
