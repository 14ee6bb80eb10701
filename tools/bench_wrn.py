#!/usr/bin/env python3
"""Time the ClassificationTrainer step of the WRN-28-10 CIFAR-100 configs (cfg/cifar100/wrn_28_10/config1.json and
config5.json plans) at batch 128 on 32x32 inputs: teacher eval forward, student train forward, KLDiv(T=5), backward, SGD.

    python tools/bench_wrn.py [--plan c1|c5] [--steps 20] [--warmup 5] [--batch 128] [--dtype fp32|bf16] [--direct]

--dtype bf16 asks DepthwiseStudent for the bf16 module graph (bf16 activations and hints, fp32 parameters and logits); the JSON
line then also counts the padding copies of one step (nn_hip._nhwc_padded: a tensor whose channel count is no multiple of the
64-channel K granule and whose producer left no zero tail).

--direct builds the same network from the NCHW small-shape modules (nn_hip.Conv2d / BatchNorm2d: kd_conv2d_direct_*,
kd_bn2d_*) for comparison.  Prints one JSON line: ms/step, img/s and TFLOP/s against the 157.3 TFLOP/s fp32 matrix peak.
FLOPs are counted algorithmically: 2 * MACs of every conv / linear of the teacher forward, the student forward, and the
student's input and weight gradients where autograd computes them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_FP32 = 157.3e12
PLANS = {
    "c1": {"hint": ["block3.layer.0", "block3.layer.1"], "unfreeze": ["block3.layer.0", "block3.layer.1"],
           "pruning_plan": ["block3.layer.0.conv2", "block3.layer.1.conv2"]},
    "c5": {"hint": ["block3"], "unfreeze": ["block2"],
           "pruning_plan": ["block2.layer.0.conv2", "block2.layer.1.conv1", "block2.layer.1.conv2", "block2.layer.2.conv1",
                            "block2.layer.2.conv2"]},
}


def build(direct):
    import importlib
    from kdcc_amd import nn_hip
    W = importlib.import_module("kdcc_amd.models.cifar_models.wrn")
    if direct:
        W.Conv2dNHWC, W.BatchNorm2dNHWC = nn_hip.Conv2d, nn_hip.BatchNorm2d
    try:
        return W.wrn(depth=28, widen_factor=10, num_classes=100)
    finally:
        W.Conv2dNHWC, W.BatchNorm2dNHWC = nn_hip.Conv2dNHWC, nn_hip.BatchNorm2dNHWC


def conv_flops(model, x, train_names):
    """(forward FLOPs, backward FLOPs) of one network: forward hooks record every conv / linear's MACs."""
    fwd, bwd, seen = [0.0], [0.0], [False]
    hooks = []

    def hook(m, inp, out, name=None):
        if isinstance(m, torch.nn.Conv2d):
            macs = out.numel() * m.in_channels // m.groups * m.kernel_size[0] * m.kernel_size[1]
        else:
            macs = out.numel() * m.in_features
        fwd[0] += 2.0 * macs
        if any(name == t or name.startswith(t + ".") for t in train_names):
            seen[0] = True
            bwd[0] += 4.0 * macs      # input gradient + weight gradient
        elif seen[0]:
            bwd[0] += 2.0 * macs      # a frozen layer behind a trained one: input gradient only
    for name, m in model.named_modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            hooks.append(m.register_forward_hook(lambda m, i, o, name=name: hook(m, i, o, name)))
    with torch.enable_grad():        # (the module path: the fused eval blocks call their convs' kernels, not the modules)
        model(x)
    for h in hooks:
        h.remove()
    return fwd[0], bwd[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", choices=sorted(PLANS), default="c1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--direct", action="store_true")
    a = ap.parse_args()
    if a.direct and a.dtype != "fp32":
        ap.error("--direct (the NCHW small-shape modules) is fp32 only")
    import kdcc_amd  # noqa: F401
    from kdcc_amd import losses, nn_hip
    from kdcc_amd.models.students import DepthwiseStudent
    torch.manual_seed(0)
    teacher = build(a.direct).cuda().eval()
    model = DepthwiseStudent(teacher, None, **({"dtype": torch.bfloat16} if a.dtype == "bf16" else {}))
    plan = PLANS[a.plan]
    model.replace([{"name": n, "epoch": 1} for n in plan["pruning_plan"]], kernel_size=3, padding=1, dilation=1)
    model.register_hint_layers(plan["hint"])
    model.unfreeze(plan["unfreeze"])
    model.train()
    opt = torch.optim.SGD([p for p in model.student.parameters() if p.requires_grad], lr=0.1)
    kd = losses.KLDivergenceLoss(temperature=5)
    x = torch.randn((a.batch, 3, 32, 32), device="cuda")
    # algorithmic work: student backward reaches down to the first trainable block
    xm = x.to(dtype=model.module_dtype, memory_format=torch.channels_last) if a.dtype == "bf16" else x
    f_t, _ = conv_flops(model.teacher, xm, [])
    f_s, b_s = conv_flops(model.student, xm, plan["unfreeze"])
    first = min(n for n, p in model.student.named_parameters() if p.requires_grad)
    flops = f_t + f_s + b_s

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
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    wall = time.perf_counter() - t0
    copies, pad = [], nn_hip._nhwc_padded       # one more step, untimed, with the padding copies counted
    nn_hip._nhwc_padded = lambda t, cpad: (copies.append(f"{t.shape[1]}->{cpad}"), pad(t, cpad))[1]
    try:
        step()
        torch.cuda.synchronize()
    finally:
        nn_hip._nhwc_padded = pad
    print(json.dumps({"tool": "bench_wrn", "plan": a.plan, "path": "direct_nchw" if a.direct else "nhwc_mfma", "dtype": a.dtype, "batch": a.batch,
                      "steps": a.steps, "ms_per_step": round(ms, 3), "img_per_s": round(a.batch * 1e3 / ms, 1),
                      "tflop_per_step": round(flops / 1e12, 4), "tflops": round(flops / ms / 1e9, 2),
                      "pct_fp32_peak": round(100.0 * flops / (ms * 1e-3) / PEAK_FP32, 2), "first_trainable": first,
                      "loss": float(loss.detach()), "wall_s": round(wall, 2), "padding_copies_per_step": len(copies),
                      "padding_copies": {k: copies.count(k) for k in sorted(set(copies))}}))


if __name__ == "__main__":
    main()
