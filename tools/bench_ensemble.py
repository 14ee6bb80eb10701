#!/usr/bin/env python3
"""Timing only (not on the test path): the ensemble step's criterion and the whole EnsembleTrainer step.

  * criterion, K = 5 members + the teacher (6 targets), labels present, at (128,100) logits (the CIFAR-100 step) and at
    (8,19,512,1024) channels-last: the one-pass kd_kldiv_multi call behind EnsembleTrainer's autograd Function, forward + backward,
    against -- in the same process, on the same tensors -- the composition of the existing modules (six KLDivergenceLoss + one
    CrossEntropyLoss2d, weighted sum, backward into one gradient).  The composition is timed five times; the fused call must not be
    slower than its median by more than its own min-max spread.  At the large shape the achieved bytes/s of the raw call against the
    (n_t + 1) reads + 1 write it needs;
  * one ensemble step of WRN-28-10, batch 128, K = 5 members of the config-5-shaped plan (randomly initialised, torch.manual_seed):
    ms per step and its split into member forwards / teacher forward / student forward + criterion + backward + SGD / criterion.

    python tools/bench_ensemble.py [--iters 30] [--warmup 5] [--steps 10] [--skip-step]

Prints one JSON line per measurement; exit status 1 when the fused criterion is slower than the allowance."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench_criteria import timeit  # noqa: E402
from bench_wrn import PLANS  # noqa: E402

K = 5


def criterion_case(name, shape, fmt, T, a):
    from kdcc_amd import losses, ops
    from kdcc_amd.trainer.ensemble_trainer import _EnsembleCriterion
    gen = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda: (torch.randn(shape, device="cuda", generator=gen) * 3).contiguous(memory_format=fmt)
    s = mk().requires_grad_(True)
    ts = [mk() for _ in range(K + 1)]
    w = [1.0] * (K + 1)
    labels = torch.randint(0, shape[1], (shape[0],) + tuple(shape[2:]), device="cuda", generator=gen)
    labels.view(-1)[::17] = 255
    kld, ce = losses.KLDivergenceLoss(temperature=T), losses.CrossEntropyLoss2d(ignore_index=255)

    def fused():
        s.grad = None
        total, _, _ = _EnsembleCriterion.apply(s, labels, float(T), 255, 1.0, w, *ts)
        total.backward()

    def composed():
        s.grad = None
        kd = 0
        for t in ts:
            kd = kd + kld(s, t)
        (kd / (K + 1) + ce(s, labels)).backward()

    def raw():
        ops.kldiv_multi(s.detach(), ts, w, T, labels, 255)

    fused(); gf = s.grad.clone()
    composed(); gc = s.grad.clone()
    rel = float((gf - gc).norm() / gc.norm())
    base = [timeit(composed, a.iters, a.warmup)[0] for _ in range(5)]
    fus = [timeit(fused, a.iters, a.warmup)[0] for _ in range(5)]
    # alternate once more so neither side owns the warmer clock
    base.append(timeit(composed, a.iters, a.warmup)[0]); base.pop(0)
    raw_med, raw_min = timeit(raw, a.iters, a.warmup)
    base_med, fus_med = sorted(base)[2], sorted(fus)[2]
    spread = max(base) - min(base)
    nbytes = (K + 3) * s.numel() * 4 + 2 * labels.numel() * 8
    ok = fus_med <= base_med + spread
    print(json.dumps({"tool": "bench_ensemble", "case": name, "shape": list(shape), "targets": K + 1, "T": T,
                      "composed_ms": [round(v, 4) for v in base], "composed_median_ms": round(base_med, 4),
                      "composed_spread_ms": round(spread, 4), "fused_ms": [round(v, 4) for v in fus],
                      "fused_median_ms": round(fus_med, 4), "speedup": round(base_med / fus_med, 2), "not_slower": bool(ok),
                      "raw_call_median_ms": round(raw_med, 4), "raw_call_min_ms": round(raw_min, 4),
                      "raw_call_GBps": round(nbytes / raw_med / 1e6, 1), "grad_rel_diff": rel}), flush=True)
    return ok


def ensemble_step(a):
    from kdcc_amd import losses
    from kdcc_amd.models.cifar_models import wrn
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer.ensemble_trainer import WEIGHT, _EnsembleCriterion
    torch.manual_seed(0)
    teacher = wrn(depth=28, widen_factor=10, num_classes=100).cuda().eval()
    model = DepthwiseStudent(teacher, None)
    members = []
    for _ in range(K):                                   # what resume_ensemble leaves behind: a copy of the student with the plan applied
        model.replace([{"name": n, "epoch": 1} for n in PLANS["c5"]["pruning_plan"]], kernel_size=3, padding=1, dilation=1)
        m = copy.deepcopy(model.student).eval()
        for p in m.parameters():
            p.requires_grad = False
        members.append(m)
        model.reset()
    for p in model.student.parameters():
        p.requires_grad = True
    model.train()
    opt = torch.optim.SGD(model.student.parameters(), lr=0.1)
    x = torch.randn((128, 3, 32, 32), device="cuda")
    y = torch.randint(0, 100, (128,), device="cuda")
    T, w = 1.0, [float(WEIGHT)] * K + [1.0]
    ev = lambda: torch.cuda.Event(enable_timing=True)
    parts = {"members_fwd": 0.0, "teacher_fwd": 0.0, "student_fwd": 0.0, "criterion": 0.0, "backward_sgd": 0.0}

    def step(record):
        marks = [ev() for _ in range(6)]
        marks[0].record()
        with torch.no_grad():
            outs = [m(x) for m in members]
        marks[1].record()
        with torch.no_grad():
            t = model.teacher(x)
        marks[2].record()
        s = model.student(x)
        marks[3].record()
        total, _, _ = _EnsembleCriterion.apply(s, y, T, 255, 1.0, w, *outs, t)
        marks[4].record()
        total.backward()
        opt.step()
        opt.zero_grad()
        marks[5].record()
        if record:
            torch.cuda.synchronize()
            for k, i in zip(parts, range(5)):
                parts[k] += marks[i].elapsed_time(marks[i + 1])
    for _ in range(a.warmup):
        step(False)
    torch.cuda.synchronize()
    e0, e1 = ev(), ev()
    e0.record()
    for _ in range(a.steps):
        step(False)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    for _ in range(a.steps):
        step(True)
    print(json.dumps({"tool": "bench_ensemble", "case": "wrn28_10_step", "batch": 128, "members": K, "steps": a.steps,
                      "ms_per_step": round(ms, 3), "img_per_s": round(128e3 / ms, 1),
                      "split_ms": {k: round(v / a.steps, 3) for k, v in parts.items()},
                      "member_fwd_ms_each": round(parts["members_fwd"] / a.steps / K, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    import kdcc_amd  # noqa: F401
    torch.cuda.set_device(0)
    ok = criterion_case("cifar100_logits", (128, 100), torch.contiguous_format, 1.0, a)
    ok = criterion_case("segmentation_logits", (8, 19, 512, 1024), torch.channels_last, 1.0, a) and ok
    if not a.skip_step:
        ensemble_step(a)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
