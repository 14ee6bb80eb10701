#!/usr/bin/env python3
"""Generate tests/golden/ensemble.npz from the REFERENCE's own EnsembleTrainer and criteria (CPU, fp32).

Runs only in the build container, like tools/make_golden_wrn.py, whose import recipe, reduced WRN, plans and batches it reuses (it
imports the reference, which does not exist on the GPU box and must never travel).  Only arrays are written:
  * crit2d / crit4d, T in {1, 5}: student logits (8,100) / (2,19,8,16), three target logit tensors with weights (1, 2, 0.5), labels
    (some 255 in the 4-D case): every KLDivergenceLoss(T)(s, t_k), their weighted mean, CrossEntropyLoss2d(s, labels), the sum of
    the two and its autograd gradient;
  * two ensemble members: DepthwiseStudent over the seeded reduced WRN ('wrn.') with the plans c1 / c5 applied, the whole student
    filled under 'ens.m0.' / 'ens.m1.', saved as {'config': plain dict, 'epoch': 1, 'state_dict', 'monitor_best'} in a temporary
    directory -- seeded, not trained, so the tests rebuild bit-identical checkpoints without shipping weights;
  * EnsembleTrainer over those two checkpoints: ensemble_predict on the first batch, the _train_epoch(1) log over the three
    trainer batches, 64 seeded projections of every student parameter afterwards, and the _test_epoch log over the same batches.

    cd /path/to/reference && python3 /path/to/repo/tools/make_golden_ensemble.py
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                   # noqa: E402  (stubs, paths, DepthwiseStudent, save)
import make_golden_wrn as mw                               # noqa: E402  (SMALL, PLANS, wrn_config, trainer_batches)

import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402

from models.cifar_models.wrn import wrn as ref_wrn         # noqa: E402
from _seeded import seeded_fill_, seeded_input             # noqa: E402
from _wrnref import project                                # noqa: E402

WEIGHTS = (1.0, 2.0, 0.5)
MEMBER_PLANS = ("c1", "c5")


def crit_inputs(tag):
    if tag == "crit2d":
        shape, labels = (8, 100), torch.randint(0, 100, (8,), generator=torch.Generator().manual_seed(41))
    else:
        shape, labels = (2, 19, 8, 16), torch.randint(0, 19, (2, 8, 16), generator=torch.Generator().manual_seed(42))
        labels[:, :2] = 255
        labels[1, 5, 3:9] = 255
    s = seeded_input(f"ens.{tag}.s", shape, 2.0)
    ts = [seeded_input(f"ens.{tag}.t{k}", shape, 2.0) for k in range(len(WEIGHTS))]
    return s, ts, labels


def g_criterion(out):
    import losses as ref_losses
    for tag in ("crit2d", "crit4d"):
        s0, ts, labels = crit_inputs(tag)
        out[f"{tag}.s"], out[f"{tag}.labels"], out[f"{tag}.w"] = s0, labels, np.array(WEIGHTS)
        for k, t in enumerate(ts):
            out[f"{tag}.t{k}"] = t
        for T in (1, 5):
            s = s0.clone().requires_grad_(True)
            kld = ref_losses.KLDivergenceLoss(temperature=T)
            each = [kld(s, t) for t in ts]
            kd = sum(w * e for w, e in zip(WEIGHTS, each)) / sum(WEIGHTS)
            sup = ref_losses.CrossEntropyLoss2d(ignore_index=255)(s, labels)
            total = kd + sup
            total.backward()
            out[f"{tag}_T{T}.kd_each"] = np.array([e.item() for e in each], dtype=np.float64)
            out[f"{tag}_T{T}.kd"] = np.float64(kd.item())
            out[f"{tag}_T{T}.sup"] = np.float64(sup.item())
            out[f"{tag}_T{T}.loss"] = np.float64(total.item())
            out[f"{tag}_T{T}.grad"] = s.grad


def member_checkpoint(index, plan, save_dir):
    """One seeded ensemble member, saved the way BaseTrainer._save_checkpoint does but with a plain-dict config."""
    cfgd = mw.wrn_config(plan, save_dir)
    teacher = ref_wrn(**mw.SMALL)
    seeded_fill_(teacher, "wrn.")
    teacher.eval()
    model = mg.DepthwiseStudent(teacher, cfgd)
    model.replace(cfgd["pruning"]["pruning_plan"], **cfgd["pruning"]["args"])
    seeded_fill_(model.student, f"ens.m{index}.")
    path = os.path.join(save_dir, f"member{index}.pth")
    torch.save({"config": cfgd, "epoch": 1, "state_dict": model.state_dict(), "monitor_best": 0}, path)
    return path


def ensemble_config(save_dir, paths):
    cfgd = mw.wrn_config("c5", save_dir)
    cfgd["name"] = "golden_ensemble"
    cfgd["trainer"]["name"] = "EnsembleTrainer"
    cfgd["trainer"]["resume_paths"] = list(paths)
    return cfgd


def g_trainer(out):
    from parse_config import ConfigParser
    from trainer import EnsembleTrainer
    from utils import WeightScheduler
    from utils import optim as ref_optim
    import losses as ref_losses
    import models.metric as ref_metric
    tmp = tempfile.mkdtemp(prefix="kdgold_ens_")
    paths = [member_checkpoint(i, plan, tmp) for i, plan in enumerate(MEMBER_PLANS)]
    config = ConfigParser(ensemble_config(tmp, paths), run_id="ens")
    teacher = ref_wrn(**mw.SMALL)
    seeded_fill_(teacher, "wrn.")
    teacher.eval()
    model = mg.DepthwiseStudent(teacher, config)
    crit = [config.init_obj(k, ref_losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(ref_metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", ref_optim, model.student.parameters())
    sched = config.init_obj("lr_scheduler", ref_optim.lr_scheduler, opt)
    batches = mw.trainer_batches()
    tr = EnsembleTrainer(model, crit, metrics, opt, config, batches, batches, sched, WeightScheduler(config["weight_scheduler"]))
    out["n_members"] = np.int64(len(tr.models))
    out["quirk:block1.layer.0.conv1.weight"] = project(model.student.block1.layer[0].conv1.weight.data, "block1.layer.0.conv1.weight")
    out["predict"] = tr.ensemble_predict(batches[0][0])
    log = tr._train_epoch(1)
    out["train_keys"] = np.array(sorted(log))
    for k, v in log.items():
        out[f"train:{k}"] = np.float64(v)
    for n, p in model.student.named_parameters():
        out[f"param:{n}"] = project(p.data, n)
    test_log = tr._test_epoch(1)
    out["test_keys"] = np.array(sorted(test_log))
    for k, v in test_log.items():
        out[f"test:{k}"] = np.float64(v)


if __name__ == "__main__":
    torch.manual_seed(0)
    out = {}
    g_criterion(out)
    g_trainer(out)
    mg.save("ensemble", **out)
