#!/usr/bin/env python3
"""Generate tests/golden/analysis.npz by running the REFERENCE's layer-compressibility analysis itself (CPU, fp32):
AnalysisStudent.replace -> one forward / hint-loss backward per probed layer, and one AnalysisTrainer._train_epoch of three RAdam
steps.  Import recipe and the neutralised hard-coded .cuda() calls come from tools/make_golden.py; the one addition
is RandomMask2d's `torch.cuda.FloatTensor(mask)`, redirected to a host tensor for the duration of the run.  Only data is written.

    python3 tools/make_golden_analysis.py

Seeds: numpy and torch are seeded with SEED + i before the i-th replace() (the mask comes from numpy's global state); the new
1x1 is then overwritten by tests/_seeded.py under the key `student.<layer>.2.` so that both sides hold the same weights without
shipping a 512 x 512 matrix.
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                                # noqa: E402  (stubs, sys.path, .cuda() neutralised)

import numpy as np                                                       # noqa: E402
import torch                                                             # noqa: E402

torch.cuda.FloatTensor = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32).copy())

from models.students import AnalysisStudent                             # noqa: E402
from _seeded import seeded_fill_, seeded_input, summarize               # noqa: E402

SEED = 1234
LAYERS = ["mod4.block2.convs.conv2", "aspp.features.1.0"]
DROPRATE = 0.85
HW, BATCH = (64, 128), 2
LR = 1e-3


def _batch(i):
    x = seeded_input(f"analysis.x{i}", (BATCH, 3) + HW)
    t = torch.randint(0, 19, (BATCH,) + HW, generator=torch.Generator().manual_seed(300 + i))
    t[:, :4] = 255
    return x, t


def _replace(model, name, i):
    np.random.seed(SEED + i)
    torch.manual_seed(SEED + i)
    model.replace([name], droprate=DROPRATE)
    blk = model.get_block(name, model.student)
    seeded_fill_(blk[2], f"student.{name}.2.")
    return blk


def main():
    from parse_config import ConfigParser
    from trainer import AnalysisTrainer
    from utils import WeightScheduler
    from utils import optim as ref_optim
    ref_losses = mg.ref_losses
    out = {"layers": np.array(LAYERS), "droprate": DROPRATE, "seed": SEED, "lr": LR}
    teacher = mg.DeepWV3Plus(num_classes=19)
    seeded_fill_(teacher, "teacher.")
    teacher.eval()

    # ---- one step per probed layer
    ce, kd_c, hint_c = ref_losses.CrossEntropyLoss2d(ignore_index=255), ref_losses.MSELoss("mean", 1), ref_losses.MSELoss("mean", 1000)
    x, t = _batch(0)
    out["target0"] = t.numpy().astype(np.uint8)
    for i, name in enumerate(LAYERS):
        model = AnalysisStudent(teacher, None)
        blk = _replace(model, name, i)
        model.register_hint_layers([name])
        trainable = [n for n, p in model.student.named_parameters() if p.requires_grad]
        assert trainable == [name + ".2.weight"], trainable
        st, tc = model(x)
        hint = sum(hint_c(a, b) for a, b in zip(model.student_hidden_outputs, model.teacher_hidden_outputs))
        hint.backward()
        key = f"step{i}"
        out[key + ".mask"] = blk[1].mask.reshape(-1).numpy().astype(np.uint8)
        out[key + ".block_out"] = summarize(model.student_hidden_outputs[0])
        out[key + ".teacher_hint"] = summarize(model.teacher_hidden_outputs[0])
        out[key + ".student_logits"] = summarize(st)
        out[key + ".teacher_logits"] = summarize(tc)
        out[key + ".hint_loss"] = np.float64(hint.item())
        out[key + ".supervised_loss"] = np.float64(ce(st, t.clone()).item())
        out[key + ".kd_loss"] = np.float64(kd_c(st, tc).item())
        out[key + ".teacher_loss"] = np.float64(ce(tc, t.clone()).item())
        g = blk[2].weight.grad
        out[key + ".grad"] = summarize(g)
        dropped = blk[1].mask.reshape(-1) == 0
        out[key + ".grad_dropped_absmax"] = np.float64(g[:, dropped].abs().max().item())

    # ---- AnalysisTrainer._train_epoch: len_epoch + 1 = 3 iterations, RAdam
    name = LAYERS[0]
    cfgd = mg.trainer_config([], lr=LR, len_epoch=2, save_dir=tempfile.mkdtemp(prefix="kdgold_"))
    cfgd["trainer"]["name"] = "AnalysisTrainer"
    cfgd["trainer"]["epochs"] = 2
    cfgd["layer_compressible"] = [{"layer_name": name, "lrs": [LR], "args": {"droprate": DROPRATE}}]
    config = ConfigParser(cfgd, run_id="a")
    model = AnalysisStudent(teacher, config)
    crit = [config.init_obj(k, ref_losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    opt = config.init_obj("optimizer", ref_optim, model.student.parameters())
    sched = config.init_obj("lr_scheduler", ref_optim.lr_scheduler, opt)
    batches = [_batch(10 + i) for i in range(3)]
    tr = AnalysisTrainer(model, crit, [], opt, config, [(a, b.clone()) for a, b in batches], None, sched,
                         WeightScheduler(config["weight_scheduler"]))
    blk = _replace(model, name, 7)                     # what AnalysisTrainer.train() does before its epochs (:22-32)
    model.register_hint_layers([name])
    tr.reset_scheduler()
    tr.create_new_optimizer()
    for group in tr.optimizer.param_groups:
        group["lr"] = LR
    log = tr._train_epoch(1, lr=LR, layer_name=name)
    out["epoch.layer"] = np.array(name)
    out["epoch.mask"] = blk[1].mask.reshape(-1).numpy().astype(np.uint8)
    out["epoch.targets"] = np.stack([b.numpy() for _, b in batches]).astype(np.uint8)
    for k, v in log.items():
        out["epoch.log:" + k] = np.float64(v)
    out["epoch.weight"] = summarize(blk[2].weight.data)
    mg.save("analysis", **out)


if __name__ == "__main__":
    main()
