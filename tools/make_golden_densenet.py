#!/usr/bin/env python3
"""Generate tests/golden/densenet_keys.json and tests/golden/densenet.npz from the REFERENCE's own CIFAR DenseNet (CPU).

Runs only in the build container, like tools/make_golden_wrn.py, whose recipe it follows (it imports the reference, which does
not exist on the GPU box and must never travel).  Only data is written:
  * densenet_keys.json: state-dict key -> shape of densenet121(), and its parameter count;
  * densenet.npz, on a reduced DenseNet (growth 32, blocks (2, 2, 2, 2), 64 stem filters: the last block runs at 2x2 pixels,
    M = 32 at batch 8, less than one 128-pixel partial of the BN reduction), seeded weights (tests/_seeded.py), batch 8:
      - teacher eval logits; student (the same weights) train-mode logits, running statistics after that forward, the
        KLDiv(T=5) loss against the teacher and every parameter gradient (as 64 seeded projections, tests/_wrnref.py);
      - ClassificationTrainer._train_epoch(1) (3 SGD steps, lr 0.1) for a config-4-shaped plan
        (features.denseblock1.denselayer{1,2}.conv2 replaced, hinted, unfrozen): the logged losses and the trainable parameters.
    Every stored tensor `name` comes with `tol:name`: the rel-L2 distance of the reference's fp32 result from the same run in
    fp64 (for a logged loss: the relative difference).  Train-mode BN over 32 values is ill-conditioned, so this -- not a guess
    -- is what the tests scale their bounds by (max(1e-3, 3 x tol)).  No tol may exceed 2e-2: the seed tags in TAGS are tried in
    order until none does, and the one used is stored as `tag` (the tests fill their models with it).  The committed file was
    made with the first tag, 'dn.' (largest tol 1.9e-4, grad:features.norm0.weight).

    cd /path/to/reference && python3 /path/to/repo/tools/make_golden_densenet.py
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

from models.cifar_models.densenet import DenseNet as RefDenseNet, densenet121 as ref_densenet121   # noqa: E402
from _seeded import seeded_fill_, seeded_input             # noqa: E402
from _densenetref import SMALL, project, rel_l2            # noqa: E402

TAGS = ["dn.", "dn1.", "dn2.", "dn3."]
TOL_MAX = 2e-2
PLAN = ["features.denseblock1.denselayer1.conv2", "features.denseblock1.denselayer2.conv2"]


def densenet_config(save_dir):
    cfgd = mg.trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
    cfgd.update(name="golden_densenet", teacher={"type": "DenseNet", "args": dict(SMALL)}, optimizer={"type": "SGD", "args": {"lr": 0.1}},
                kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
                hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}},
                metrics=["accuracy", "top_k_acc"],
                lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}})
    cfgd["trainer"]["name"] = "ClassificationTrainer"
    cfgd["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3},
                       **{k: [{"name": n, "epoch": 1} for n in PLAN] for k in ("hint", "unfreeze", "pruning_plan")}}
    return cfgd


def trainer_batches(tag, dtype):
    return [(seeded_input(f"{tag}tr.x{i}", (8, 3, 32, 32)).to(dtype),
             torch.randint(0, 10, (8,), generator=torch.Generator().manual_seed(300 + i))) for i in range(3)]


def g_keys():
    with torch.device("meta"):
        m = ref_densenet121()
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    path = os.path.join(mg.OUT, "densenet_keys.json")
    with open(path, "w") as f:
        json.dump({"keys": keys, "num_params": sum(p.numel() for p in m.parameters())}, f, indent=0)
    print("wrote", path)


def small_run(tag, dtype):
    import losses as ref_losses
    out = {}
    teacher = seeded_fill_(RefDenseNet(**SMALL), tag).to(dtype).eval()
    x = seeded_input(tag + "x", (8, 3, 32, 32)).to(dtype)
    with torch.no_grad():
        out["teacher_logits"] = teacher(x)
    student = copy.deepcopy(teacher).train()
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
    return out


def trainer_run(tag, dtype):
    from parse_config import ConfigParser
    from trainer import ClassificationTrainer
    from utils import WeightScheduler
    from utils import optim as ref_optim
    import losses as ref_losses
    import models.metric as ref_metric
    import models.cifar_models.densenet as ref_dn
    out = {}
    config = ConfigParser(densenet_config(tempfile.mkdtemp(prefix="kdgold_")), run_id="c4")
    teacher = seeded_fill_(config.init_obj("teacher", ref_dn), tag).to(dtype).eval()
    model = mg.DepthwiseStudent(teacher, config)
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"{tag}student.{b['name']}.").to(dtype)
    model.replace = replace_and_seed
    crit = [config.init_obj(k, ref_losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(ref_metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", ref_optim, model.student.parameters())
    sched = config.init_obj("lr_scheduler", ref_optim.lr_scheduler, opt)
    tr = ClassificationTrainer(model, crit, metrics, opt, config, trainer_batches(tag, dtype), None, sched,
                               WeightScheduler(config["weight_scheduler"]))
    log = tr._train_epoch(1)
    for k, v in log.items():
        out[f"c4:log:{k}"] = np.float64(v)
    out["c4:trainable"] = np.array(sorted(n for n, p in model.student.named_parameters() if p.requires_grad))
    for n, p in model.student.named_parameters():
        if p.requires_grad:
            out[f"c4:param:{n}"] = project(p.data, n)
    return out


def with_tols(tag):
    f32 = {**small_run(tag, torch.float32), **trainer_run(tag, torch.float32)}
    f64 = {**small_run(tag, torch.float64), **trainer_run(tag, torch.float64)}
    out, worst = dict(f32), (0.0, None)
    assert list(f32["c4:trainable"]) == list(f64["c4:trainable"])
    for k, v in f32.items():
        if k == "c4:trainable":
            continue
        a, b = torch.as_tensor(np.asarray(v.detach() if torch.is_tensor(v) else v)), torch.as_tensor(np.asarray(f64[k].detach() if torch.is_tensor(f64[k]) else f64[k]))
        tol = rel_l2(a.reshape(-1), b.reshape(-1))
        out["tol:" + k] = np.float64(tol)
        if ":log:" in k and k.split(":")[-1] not in ("loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss"):
            continue                    # (accuracy counters: stored, not bounded)
        worst = max(worst, (tol, k))
    return out, worst


if __name__ == "__main__":
    torch.manual_seed(0)
    g_keys()
    for tag in TAGS:
        out, worst = with_tols(tag)
        print(f"tag {tag!r}: largest tol {worst[0]:.3e} ({worst[1]})")
        if worst[0] <= TOL_MAX:
            break
    else:
        raise SystemExit("no seed tag keeps every tol below %g" % TOL_MAX)
    out["tag"] = np.array(tag)
    mg.save("densenet", **out)
    top = sorted(((float(v), k) for k, v in out.items() if k.startswith("tol:")), reverse=True)[:8]
    print("\n".join(f"  {k}: {v:.3e}" for v, k in top))
