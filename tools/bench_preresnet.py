#!/usr/bin/env python3
"""Measure preresnet-110 on CIFAR-100 at batch 128 (32x32 inputs), in alternating fresh processes on one box:

  nhwc    one ClassificationTrainer-shaped step (teacher eval forward, student train forward, KLDiv(T=5), backward, SGD) on the
          channels-last MFMA path with the fused BN-ReLU-pool head -- what models/cifar_models/preresnet.py builds;
  direct  the same step with the net rebuilt from the NCHW small-shape modules (nn_hip.Conv2d / BatchNorm2d: kd_conv2d_direct_*,
          kd_bn2d_*), the fastest the tree offered this net before the channels-last PreResNet;
  head    the fused head (kd_head_bn_relu_pool_fwd + _bwd, batch statistics included) against the composition it replaces --
          BatchNorm2dNHWC(relu=True), F.avg_pool2d and their backward -- at (128, 8, 8, 64) and (128, 8, 8, 256), forward + backward,
          the two alternating inside one process.

    python tools/bench_preresnet.py [--rounds 3] [--steps 20] [--warmup 5] [--batch 128] [--out FILE]

The driver never touches the GPU: it starts `--child nhwc|direct|head` processes one after the other, `--rounds` of each in
alternation, under a time limit each, stops at the first child that fails, prints every child's JSON line and one summary line
(medians), and appends them to --out.  The plan is the WRN bench's c1 shape: the last two blocks' conv2 replaced, those blocks hinted
and unfrozen."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAN = {"hint": ["layer3.16", "layer3.17"], "unfreeze": ["layer3.16", "layer3.17"], "pruning_plan": ["layer3.16.conv2", "layer3.17.conv2"]}
HEAD_SHAPES = ((128, 8, 8, 64), (128, 8, 8, 256))


def build(direct):
    import importlib
    from kdcc_amd import nn_hip
    P = importlib.import_module("kdcc_amd.models.cifar_models.preresnet")
    if direct:
        P.Conv2dNHWC, P.BatchNorm2dNHWC = nn_hip.Conv2d, nn_hip.BatchNorm2d
    try:
        return P.preresnet(depth=110, num_classes=100)
    finally:
        P.Conv2dNHWC, P.BatchNorm2dNHWC = nn_hip.Conv2dNHWC, nn_hip.BatchNorm2dNHWC


def child_step(a, direct):
    import torch
    from kdcc_amd import losses
    from kdcc_amd.models.students import DepthwiseStudent
    torch.manual_seed(0)
    teacher = build(direct).cuda().eval()
    model = DepthwiseStudent(teacher, None)
    model.replace([{"name": n, "epoch": 1} for n in PLAN["pruning_plan"]], kernel_size=3, padding=1, dilation=1)
    model.register_hint_layers(PLAN["hint"])
    model.unfreeze(PLAN["unfreeze"])
    model.train()
    opt = torch.optim.SGD([p for p in model.student.parameters() if p.requires_grad], lr=0.1)
    kd = losses.KLDivergenceLoss(temperature=5)
    x = torch.randn((a.batch, 3, 32, 32), device="cuda")

    def step():
        model.student_hidden_outputs.clear(); model.teacher_hidden_outputs.clear()
        s, t = model(x)
        loss = kd(s, t)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    print(json.dumps({"tool": "bench_preresnet", "what": "direct_nchw" if direct else "nhwc_mfma", "batch": a.batch, "steps": a.steps,
                      "ms_per_step": round(ms, 3), "img_per_s": round(a.batch * 1e3 / ms, 1), "loss": float(loss.detach())}))


def child_head(a):
    import torch
    import torch.nn.functional as F
    from kdcc_amd import nn_hip
    iters, blocks = 200, 5
    for shape in HEAD_SHAPES:
        N, H, W, Cc = shape
        torch.manual_seed(0)
        bn = nn_hip.BatchNorm2dNHWC(Cc).cuda().train()
        relu = torch.nn.ReLU()
        x = torch.randn((N, Cc, H, W), device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gp = torch.randn((N, Cc), device="cuda")

        def fused():
            nn_hip.bn_relu_avgpool(bn, relu, x, H).backward(gp)

        def composed():
            F.avg_pool2d(bn(x, relu=True), H).flatten(1).backward(gp)
        times = {"fused": [], "composed": []}
        for _ in range(3):                  # (warm-up: code objects, the allocator's blocks, the clocks; a fresh process needs ~1 s)
            for fn in (fused, composed):
                for _ in range(iters):
                    fn()
        torch.cuda.synchronize()
        for _ in range(blocks):
            for name, fn in (("fused", fused), ("composed", composed)):
                x.grad = bn.weight.grad = bn.bias.grad = None
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / iters)
        f, c = statistics.median(times["fused"]), statistics.median(times["composed"])
        print(json.dumps({"tool": "bench_preresnet", "what": "head", "shape": list(shape), "iters": iters, "fused_us": round(f, 2),
                          "composed_us": round(c, 2), "fused_us_all": [round(t, 2) for t in times["fused"]],
                          "composed_us_all": [round(t, 2) for t in times["composed"]], "composed_over_fused": round(c / f, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out")
    ap.add_argument("--child", choices=("nhwc", "direct", "head"))
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        import kdcc_amd  # noqa: F401
        if a.child == "head":
            child_head(a)
        else:
            child_step(a, a.child == "direct")
        return 0
    lines = []
    for r in range(a.rounds):
        for what in ("nhwc", "direct", "head"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--batch", str(a.batch)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            if p.returncode != 0:
                print(f"child {what} (round {r}) exited {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
                return 1
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    rec = json.loads(ln)
                    rec["round"] = r
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
    med = lambda xs: round(statistics.median(xs), 3)
    summary = {"tool": "bench_preresnet", "what": "summary", "rounds": a.rounds, "batch": a.batch}
    for what in ("nhwc_mfma", "direct_nchw"):
        summary[what + "_ms_per_step"] = med([l["ms_per_step"] for l in lines if l["what"] == what])
    summary["direct_over_nhwc"] = round(summary["direct_nchw_ms_per_step"] / summary["nhwc_mfma_ms_per_step"], 3)
    for shape in HEAD_SHAPES:
        hs = [l for l in lines if l["what"] == "head" and tuple(l["shape"]) == shape]
        key = "head_C%d" % shape[3]
        summary[key + "_fused_us"], summary[key + "_composed_us"] = med([l["fused_us"] for l in hs]), med([l["composed_us"] for l in hs])
        summary[key + "_composed_over_fused"] = round(summary[key + "_composed_us"] / summary[key + "_fused_us"], 3)
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines + [summary]:
                f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
