#!/usr/bin/env python3
"""Timing only (not on the test path): one optimizer step() over the parameter sets of two real module trees -- WRN-28-10
(depth 28, widen 10, 100 classes) and the CIFAR ResNet-110 -- for plain SGD (lr only, what the shipped WRN configs use), SGD with
momentum 0.9 + weight decay + nesterov, and Adam; this package's classes (kd_optim_step_multi) next to torch.optim at its
default (foreach on the device), with foreach=False and with fused=True.

    python tools/bench_optim.py [--steps 30] [--repeats 5] [--warmup 5] [--out profiles/optim_step.md] [--launches]

One process.  A step is timed by the host clock from the call of step() to the end of a device synchronise (the step of the
small set is bound by its launches, which device events round a single kernel would not show); each repeat is the median of
`--steps` steps, the methods alternate inside a repeat, the table gives the median of the repeats and their spread.  Bytes/s
are the bytes the rule needs (every operand read once, every result written once: 12 B per parameter for plain SGD, 20 B with
momentum, 28 B for Adam) over that time.  --launches counts the device kernels of one step with torch.profiler, in a pass of
its own after the timing.  Prints one JSON line per row and writes the table as markdown."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

RULES = [
    ("sgd plain", "SGD", dict(lr=0.1), 12),
    ("sgd momentum+wd+nesterov", "SGD", dict(lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True), 20),
    ("adam", "Adam", dict(lr=1e-3), 28),
]
METHODS = [("kdcc", None), ("torch default", {}), ("torch foreach=False", dict(foreach=False)), ("torch fused=True", dict(fused=True))]


def shapes():
    import kdcc_amd  # noqa: F401
    from kdcc_amd.models.cifar_models import WideResNet, resnet110
    nets = {"WRN-28-10": WideResNet(depth=28, num_classes=100, widen_factor=10), "ResNet-110": resnet110()}
    return {k: [tuple(p.shape) for p in m.parameters() if p.requires_grad] for k, m in nets.items()}


def make(shapes_, gen):
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.1) for s in shapes_]
    for p in ps:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 0.01
    return ps


def one_step_ms(opt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def count_launches(opt):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.md"))
    ap.add_argument("--launches", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the device: there is nothing to fall back to"
    from kdcc_amd import _lib
    from kdcc_amd.utils import optim
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for net, shp in shapes().items():
        numel = sum(int(torch.Size(s).numel()) for s in shp)
        for rname, cname, kw, bpp in RULES:
            opts = []
            for mname, extra in METHODS:
                cls = getattr(optim, cname) if extra is None else getattr(torch.optim, cname)
                opts.append((mname, cls(make(shp, gen), **kw, **(extra or {}))))
            for _, opt in opts:
                for _ in range(a.warmup):
                    opt.step()
            reps = {m: [] for m, _ in opts}
            for _ in range(a.repeats):
                for m, opt in opts:
                    reps[m].append(median([one_step_ms(opt) for _ in range(a.steps)]))
            base = median(reps["kdcc"])
            for m, opt in opts:
                med = median(reps[m])
                row = dict(net=net, tensors=len(shp), parameters=numel, rule=rname, method=m, ms=round(med, 4), ms_min=round(min(reps[m]), 4),
                           ms_max=round(max(reps[m]), 4), GBps=round(numel * bpp / med / 1e6, 1), vs_kdcc=round(med / base, 3), launches=None)
                if m == "kdcc":
                    assert _lib.last_plumbing_kernel().startswith("optim_multi_kernel"), "the kdcc row did not run the kernel"
                rows.append((row, opt))
                print(json.dumps(row), flush=True)
            write(a.out, rows, a)
    if a.launches:
        for row, opt in rows:
            row["launches"] = count_launches(opt)
            print(json.dumps(dict(net=row["net"], rule=row["rule"], method=row["method"], launches=row["launches"])), flush=True)
        write(a.out, rows, a)


def write(path, rows, a):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("# One optimizer step: kd_optim_step_multi next to torch.optim\n\n")
        f.write(f"`python tools/bench_optim.py --steps {a.steps} --repeats {a.repeats} --warmup {a.warmup}"
                f"{' --launches' if a.launches else ''}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, one process.\n"
                "ms: host clock from the call of step() to the end of a device synchronise, median of the repeats (each the median of "
                "the steps), with the spread of the repeats.  GB/s: the bytes the rule needs (12 / 20 / 28 B per parameter) over that "
                "time -- a whole-step rate, launches and host work included, not a kernel's share of peak.  vs kdcc: that method's ms over "
                "this package's (above 1: torch is slower).  kernels per step (with --launches): the device kernels torch.profiler saw "
                "during one step() after the timing; this package's own launches are ceil(tensors / 72) for SGD and ceil(tensors / 48) "
                "for Adam, whatever else the profiler attributes to the step is counted too, in every row alike.  What the figures "
                "mean is written down in profiles/optim_step_reading.md, by hand.\n\n")
        f.write("| parameter set | rule | method | ms (min .. max) | GB/s | vs kdcc | kernels per step |\n|---|---|---|---|---|---|---|\n")
        for r, _ in rows:
            f.write(f"| {r['net']} ({r['tensors']} tensors, {r['parameters'] / 1e6:.2f} M) | {r['rule']} | {r['method']} | {r['ms']:.3f} "
                    f"({r['ms_min']:.3f} .. {r['ms_max']:.3f}) | {r['GBps']:.0f} | {r['vs_kdcc']:.2f} | "
                    f"{'not counted' if r['launches'] is None else r['launches']} |\n")


if __name__ == "__main__":
    main()
