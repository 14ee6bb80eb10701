#!/usr/bin/env python3
"""Generate tests/golden/hrnet_keys.json and tests/golden/hrnet.npz from the REFERENCE's own HighResolutionNet (CPU).

Runs only in the build container, like tools/make_golden_densenet.py, whose recipe and tolerance rule it follows (it imports the
reference, which must never travel).  The reference reads its default config with a path relative to its own root and calls
the removed NumPy name `np.int`: this tool changes into the reference's directory and aliases the name; nothing is copied.
Only data is written:
  * hrnet_keys.json: state-dict key -> shape of HighResolutionNet() (the W48 default), and its parameter count;
  * hrnet.npz, on the narrow config of tests/_hrnetref.py with seeded weights (tests/_seeded.py; no weights are stored) and a
    seeded 2 x 3 x 64 x 96 input:
      - eval-mode logits; train-mode logits with the dropout probability set to 0 (logits as the fixed 4096-element subsample
        of tests/_seeded.py sample_idx, in NCHW order; hints whole, flattened in NCHW order);
      - after the shipped plan's replacements (seeded block weights), student in eval mode as LayerwiseTrainer keeps it: the
        student and teacher hint tensors, the hint loss (MSELoss, num_classes 1000, summed over the hints), the supervised / KD / teacher
        loss terms of the step (CrossEntropyLoss2d with ignore_index 255 on seeded labels, MSELoss num_classes 1) and the gradients of
        the trainable weights (as 64 seeded projections each).
    Every stored tensor `name` comes with `tol:name`: the rel-L2 distance of the reference's fp32 result from the same run in
    fp64.  The tests bound by max(1e-3, 3 x tol).

    cd /path/to/reference && python3 /path/to/repo/tools/make_golden_hrnet.py
"""
import copy
import json
import os
import sys

import numpy as np

if not hasattr(np, "int"):
    np.int = int                                           # (the reference calls np.int, removed in NumPy 1.24)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg                                  # noqa: E402  (stubs, paths, DepthwiseStudent, save)

os.chdir(mg.REF)                                           # (seg_hrnet_ocr.py opens 'models/hrnet_ocr/config_hrnet_ocr.json')
import torch                                               # noqa: E402
from torch import nn                                       # noqa: E402

from models.hrnet_ocr.seg_hrnet_ocr import HighResolutionNet as RefHRNet   # noqa: E402
from _seeded import sample_idx                             # noqa: E402
from _hrnetref import seeded_target                        # noqa: E402
from _hrnetref import HINT_CLASSES, INPUT_SHAPE, NARROW, PLAN, PLAN_ARGS, TAG, project, rel_l2, seeded_fill_, seeded_input   # noqa: E402


def g_keys():
    with torch.device("meta"):
        m = RefHRNet()
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    path = os.path.join(mg.OUT, "hrnet_keys.json")
    with open(path, "w") as f:
        json.dump({"keys": keys, "num_params": sum(p.numel() for p in m.parameters())}, f, indent=0)
    print("wrote", path)


def run(dtype):
    out = {}
    teacher = seeded_fill_(RefHRNet(copy.deepcopy(NARROW)), TAG).to(dtype).eval()
    x = seeded_input(TAG + "x", INPUT_SHAPE).to(dtype)
    with torch.no_grad():
        out["eval_logits"] = teacher(x)
        tr = copy.deepcopy(teacher).train()
        for m in tr.modules():
            if isinstance(m, nn.Dropout2d):
                m.p = 0.0
        out["train_logits"] = tr(x)
    model = mg.DepthwiseStudent(teacher, None)
    model.replace([{"name": n, "epoch": 1} for n in PLAN], **PLAN_ARGS)
    for n in PLAN:
        seeded_fill_(model.get_block(n, model.student), f"{TAG}student.{n}.").to(dtype)
    model.register_hint_layers(PLAN)
    model.unfreeze(PLAN)
    model.student.eval()
    s, t = model(x)
    out["student_logits"], out["teacher_logits"] = s.detach(), t.detach()
    crit = mg.ref_losses.MSELoss(reduction="mean", num_classes=HINT_CLASSES)
    loss = sum(crit(a, b) for a, b in zip(model.student_hidden_outputs, model.teacher_hidden_outputs))
    loss.backward()
    out["hint_loss"] = loss.detach()
    # the other terms LayerwiseTrainer logs for the step (supervised, KD, the teacher's supervised loss), seeded labels with ignored pixels
    target = seeded_target()
    ce, kd = mg.ref_losses.CrossEntropyLoss2d(ignore_index=255), mg.ref_losses.MSELoss(reduction="mean", num_classes=1)
    with torch.no_grad():
        out["supervised_loss"], out["kd_loss"], out["teacher_loss"] = ce(s, target), kd(s, t), ce(t, target)
    for i, (a, b) in enumerate(zip(model.student_hidden_outputs, model.teacher_hidden_outputs)):
        out[f"hint_s{i}"], out[f"hint_t{i}"] = a.detach(), b.detach()
    names = sorted(n for n, p in model.student.named_parameters() if p.requires_grad)
    out["trainable"] = np.array(names)
    for n, p in model.student.named_parameters():
        if p.requires_grad:
            out["grad:" + n] = project(p.grad, n)
    return out


if __name__ == "__main__":
    torch.manual_seed(0)
    g_keys()
    f32, f64 = run(torch.float32), run(torch.float64)
    assert list(f32["trainable"]) == list(f64["trainable"])
    out = {}
    for k, v in f32.items():
        if k == "trainable":
            out[k] = v
            continue
        a, b = torch.as_tensor(np.asarray(v)).double(), torch.as_tensor(np.asarray(f64[k])).double()
        a, b = a.reshape(-1), b.reshape(-1)
        if k.endswith("logits"):                           # (a fixed subsample, tests/_seeded.py: the fixture stays small)
            idx = sample_idx(a.numel())
            a, b = a[idx], b[idx]
        out[k] = np.asarray(a.float() if a.numel() > 64 else a)
        out["tol:" + k] = np.float64(rel_l2(a, b))
    mg.save("hrnet", **out)
    for v, k in sorted(((float(v), k) for k, v in out.items() if k.startswith("tol:")), reverse=True)[:8]:
        print(f"  {k}: {v:.3e}")
