#!/usr/bin/env python3
"""Measure the fused BatchNorm -> ReLU -> MaxPool2d(2, 2) of the CIFAR VGGs (kd_bn_relu_maxpool2x2_fwd / _bwd, csrc/pool_ops.hip)
against the composition the tree had before it -- BatchNorm2dNHWC(x, relu=True) followed by F.max_pool2d(2, 2) under autograd -- at
batch 128 (32x32 inputs), on one box:

  stages  at each of vgg16_bn's five pooled stages (32x32x64, 16x16x128, 8x8x256, 4x4x512, 2x2x512), train mode: the forward alone
          and forward + backward of both versions, alternating inside one process, device events around `--iters` calls, `--blocks`
          repeats; the spread reported is max - min over a version's blocks.  The verdict per stage and pass: the fused version holds
          where its median is no more than the composition's median plus the composition's own spread;
  step    one vgg16_bn train step (forward, cross entropy, backward, SGD) as shipped (the fused tail where
          nn_hip.POOL_FUSE_MIN_ELEMENTS sends it) and on the composition, alternating in one process; the composition is reached
          through the hook fallback (a no-op forward hook on every MaxPool2d);
  trace   (needs rocprofv3) the kernel time of one forward + backward per stage and version, from `rocprofv3 --kernel-trace --stats`
          runs of their own, next to the bytes each version has to move, computed from the shapes by bytes_moved() below, and the
          share of the HBM bandwidth a float4 copy reaches on this GPU (6.29 TB/s measured, 8.0 TB/s spec).

    python tools/bench_vgg.py [--iters 200] [--blocks 5] [--steps 20] [--batch 128] [--no-trace] [--out FILE]

The driver never touches the GPU: it starts `--child ...` processes one after the other, each under a time limit, stops at the first
child that fails, prints every child's JSON line and appends them to --out."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ((32, 64), (16, 128), (8, 256), (4, 512), (2, 512))       # (map side, channels) in front of each of vgg16_bn's pools
HBM_COPY_TBS, HBM_SPEC_TBS = 6.29, 8.0


def bytes_moved(batch, side, channels):
    """Bytes each version has to move for one train-mode forward and one backward of a stage, from the shapes (fp32; per-channel
    vectors and partial sums left out).  full = the map, q = the pooled map, a quarter of it."""
    full = batch * side * side * channels * 4
    q = full // 4
    fwd_fused = full + (full + q)                           # statistics read x; the pool kernel reads x, writes y
    fwd_comp = full + (full + full) + (full + q)            # statistics; apply reads x, writes a; max_pool reads a, writes y
    bwd_fused = (full + q) + (full + q + full)              # stage 1 reads x, gy; dx reads x, gy, writes dx
    bwd_comp = (q + full) + 3 * full + (3 * full + full)    # max_pool backward reads gy (and its indices / a: left out), writes ga;
    #                                                         BN stage 1 reads ga, x, a; BN dx reads ga, x, a, writes dx
    return {"fwd_fused": fwd_fused, "fwd_composed": fwd_comp, "bwd_fused": bwd_fused, "bwd_composed": bwd_comp}


def _stage(batch, side, channels):
    import torch
    import torch.nn.functional as F
    from kdcc_amd import nn_hip
    torch.manual_seed(0)
    bn = nn_hip.BatchNorm2dNHWC(channels).cuda().train()
    relu, pool = torch.nn.ReLU(inplace=True), torch.nn.MaxPool2d(2, 2)
    x = torch.randn((batch, channels, side, side), device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gp = torch.randn((batch, channels, side // 2, side // 2), device="cuda").contiguous(memory_format=torch.channels_last)
    nn_hip.POOL_FUSE_MIN_ELEMENTS = 0           # (measure the fused kernels at every stage, whatever ships there)
    fused = lambda: nn_hip.bn_relu_maxpool(bn, relu, pool, x)
    composed = lambda: F.max_pool2d(bn(x, relu=True), 2, 2)

    def clear():
        x.grad = bn.weight.grad = bn.bias.grad = None
    return {"fused": fused, "composed": composed}, gp, clear


def child_stages(a):
    import torch
    from kdcc_amd import _lib
    for side, channels in STAGES:
        fns, gp, clear = _stage(a.batch, side, channels)
        y = fns["fused"]()
        assert _lib.last_plumbing_kernel().startswith("pool_fwd_kernel"), "the fused path was not taken"
        ref = fns["composed"]()
        assert torch.equal(y, ref) or float((y - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), "the two versions disagree"
        passes = {"fwd": lambda fn: fn(), "fwd_bwd": lambda fn: fn().backward(gp)}
        times = {(p, v): [] for p in passes for v in fns}
        for _ in range(2):                  # (warm-up: code objects, the allocator's blocks, the clocks)
            for p, run in passes.items():
                for v, fn in fns.items():
                    for _ in range(a.iters):
                        run(fn)
                    clear()
        torch.cuda.synchronize()
        for _ in range(a.blocks):
            for p, run in passes.items():
                for v, fn in fns.items():
                    clear()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        run(fn)
                    e1.record()
                    torch.cuda.synchronize()
                    times[(p, v)].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        rec = {"tool": "bench_vgg", "what": "stage", "shape": [a.batch, side, side, channels], "iters": a.iters, "blocks": a.blocks}
        for (p, v), ts in times.items():
            rec[f"{p}_{v}_us"] = round(statistics.median(ts), 2)
            rec[f"{p}_{v}_spread_us"] = round(max(ts) - min(ts), 2)
            rec[f"{p}_{v}_us_all"] = [round(t, 2) for t in ts]
        for p in passes:
            rec[f"{p}_fused_holds"] = rec[f"{p}_fused_us"] <= rec[f"{p}_composed_us"] + rec[f"{p}_composed_spread_us"]
            rec[f"{p}_composed_over_fused"] = round(rec[f"{p}_composed_us"] / rec[f"{p}_fused_us"], 3)
        print(json.dumps(rec), flush=True)


def child_step(a):
    import torch
    import torch.nn.functional as F
    from kdcc_amd.models.cifar_models import vgg16_bn
    torch.manual_seed(0)
    m = vgg16_bn(num_classes=10).cuda().train()
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    x = torch.randn((a.batch, 3, 32, 32), device="cuda")
    t = torch.arange(a.batch, device="cuda") % 10
    pools = [c for c in m.features if isinstance(c, torch.nn.MaxPool2d)]

    def step():
        loss = F.cross_entropy(m(x), t)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss
    times = {"fused": [], "composed": []}
    for measured in (False,) + (True,) * a.blocks:
        for v in times:
            hooks = [p.register_forward_hook(lambda mod, i, o: None) for p in pools] if v == "composed" else []
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                loss = step()
            e1.record()
            torch.cuda.synchronize()
            if measured:
                times[v].append(e0.elapsed_time(e1) / a.steps)
            for h in hooks:
                h.remove()
    rec = {"tool": "bench_vgg", "what": "step", "net": "vgg16_bn", "batch": a.batch, "steps": a.steps, "blocks": a.blocks,
           "loss": float(loss.detach())}
    for v, ts in times.items():
        rec[f"{v}_ms"] = round(statistics.median(ts), 3)
        rec[f"{v}_spread_ms"] = round(max(ts) - min(ts), 3)
        rec[f"{v}_ms_all"] = [round(t, 3) for t in ts]
    rec["composed_over_fused"] = round(rec["composed_ms"] / rec["fused_ms"], 3)
    print(json.dumps(rec), flush=True)


def child_trace(a):
    """`--trace-iters` forward + backward calls of one version at one stage and nothing else in the loop: what rocprofv3 watches."""
    import torch
    side, channels = STAGES[a.stage]
    fns, gp, clear = _stage(a.batch, side, channels)
    for _ in range(a.trace_iters):
        fns[a.version]().backward(gp)
        clear()
    torch.cuda.synchronize()


def short_name(name):
    """A kernel's demangled signature without its return type, anonymous namespaces and argument list."""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "", 1).strip()
    depth = 0
    for i, ch in enumerate(name):           # cut at the argument list: the first "(" outside template brackets
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i][:100]
    return name[:100]


def kernel_us(stats_dir, iters):
    """Sum over the kernels of the loop (those called at least `iters` times) of their total time, per iteration, in us; and their
    names with the calls per iteration."""
    files = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        print("no kernel_stats.csv under", stats_dir, ":", [os.path.relpath(os.path.join(r, f), stats_dir)
                                                            for r, _, fs in os.walk(stats_dir) for f in fs][:20], file=sys.stderr)
        return None, {}
    total, names = 0.0, {}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            calls = int(row["Calls"])
            if calls >= iters:
                total += float(row["TotalDurationNs"])
                names[short_name(row["Name"])] = round(calls / iters, 2)
    return total / iters / 1e3, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--trace-iters", type=int, default=50)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--child", choices=("stages", "step", "trace"))
    ap.add_argument("--stage", type=int, default=0)
    ap.add_argument("--version", choices=("fused", "composed"), default="fused")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        import kdcc_amd  # noqa: F401
        {"stages": child_stages, "step": child_step, "trace": child_trace}[a.child](a)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--iters", str(a.iters), "--blocks", str(a.blocks),
          "--steps", str(a.steps), "--trace-iters", str(a.trace_iters)]
    lines = []

    def run(cmd, what):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        if p.returncode != 0:
            print(f"child {what} exited {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return False
        for ln in p.stdout.splitlines():
            if ln.startswith('{"tool"'):
                lines.append(json.loads(ln))
                print(ln, flush=True)
        return True
    ok = run(me + ["--child", "stages"], "stages") and run(me + ["--child", "step"], "step")
    prof = shutil.which("rocprofv3")
    if ok and not a.no_trace and prof:
        for i, (side, channels) in enumerate(STAGES):
            rec = {"tool": "bench_vgg", "what": "trace", "shape": [a.batch, side, side, channels], "iters": a.trace_iters,
                   "bytes": bytes_moved(a.batch, side, channels)}
            for v in ("fused", "composed"):
                d = tempfile.mkdtemp(prefix="bench_vgg_")
                ok = run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "trace", "--stage", str(i), "--version", v],
                         f"trace {i} {v}")
                if not ok:
                    break
                us, names = kernel_us(d, a.trace_iters)
                shutil.rmtree(d, ignore_errors=True)
                rec[f"{v}_kernel_us"], rec[f"{v}_kernels"] = (None if us is None else round(us, 2)), names
                if us:
                    b = rec["bytes"][f"fwd_{v}"] + rec["bytes"][f"bwd_{v}"]
                    rec[f"{v}_TBs"] = round(b / us / 1e6, 3)
                    rec[f"{v}_share_of_copy_bw"] = round(b / us / 1e6 / HBM_COPY_TBS, 3)
            if not ok:
                break
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    elif ok and not a.no_trace:
        print("rocprofv3 not found: kernel times not measured", file=sys.stderr)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
