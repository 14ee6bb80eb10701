#!/usr/bin/env python3
"""Measure the dropout pass (kd_dropout_nhwc, csrc/dropout.hip) and what it costs a Wide-ResNet training step, in fresh processes on
one box:

  kernel  kd_dropout_nhwc out of place and in place, and kd_copy_cast -- the plain pass over the same bytes -- on the same tensors,
          fp32 and bf16, at the activations WRN-28-10 drops at batch 128: 32x32x160, 16x16x320, 8x8x640 (bf16: the 160 channels in
          their 192-channel padded buffer, as the model holds them).  The three alternate in blocks inside one process;
  step    one WRN-28-10 training step (train-mode forward, cross entropy, backward, SGD) at batch 128, fp32 or bf16, with dropRate
          0.3 or 0, one process each, alternating.

    python tools/bench_dropout.py [--rounds 3] [--steps 20] [--warmup 5] [--batch 128] [--out profiles/dropout]

The driver never touches the GPU: it starts the children one after the other, `--rounds` of each in alternation, under a time limit
each, stops at the first child that fails, prints every child's JSON line, appends them to <out>.jsonl and writes the tables of
medians between the `measured` markers of <out>.md (the prose around them is kept).  Times are device events around a loop that ends
in a synchronise: call times.  At the small shapes a call is shorter than its enqueue, so the kernel child also reports the bytes a
call moves; kernel times proper come from a trace taken in a run of its own (the command is in the profile)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((128, 32, 32, 160), (128, 16, 16, 320), (128, 8, 8, 640))
BEGIN, END = "<!-- measured: begin -->", "<!-- measured: end -->"


def child_kernel(a):
    import torch
    from kdcc_amd import nn_hip, ops
    blocks = 5
    configs = [(dtype, dname, shape) for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")) for shape in SHAPES]
    for dtype, dname, shape in (configs if a.only is None else [configs[a.only]]):      # (--only: one config, for a trace of its own)
        torch.manual_seed(0)
        x = nn_hip.new_padded(shape, "cuda", dtype)
        y = nn_hip.new_padded(shape, "cuda", dtype)
        z = nn_hip.new_padded(shape, "cuda", dtype)          # (the in-place call's own tensor: its values grow call by call)
        x.copy_(torch.randn(shape, device="cuda").to(dtype))
        z.copy_(x)
        xn, yn = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
        nbytes = 2 * x.numel() * x.element_size()
        iters = max(50, min(5000, int(a.kernel_bytes / nbytes)))
        calls = {"dropout": lambda: ops.dropout_nhwc(x, 0.3, 123, 0, out=y),
                 "dropout_inplace": lambda: ops.dropout_nhwc(z, 0.3, 123, 0, out=z),
                 "copy_cast": lambda: ops.copy_cast(xn, yn)}
        times = {k: [] for k in calls}
        for fn in calls.values():            # (warm-up: code objects, the clocks)
            for _ in range(iters):
                fn()
        torch.cuda.synchronize()
        for _ in range(blocks):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / iters)
        rec = {"tool": "bench_dropout", "what": "kernel", "dtype": dname, "shape": list(shape), "ld": x.stride(2), "iters": iters,
               "bytes_per_call": nbytes}
        for name, ts in times.items():
            rec[name + "_us"] = round(statistics.median(ts), 2)
            rec[name + "_us_all"] = [round(t, 2) for t in ts]
            rec[name + "_GBps"] = round(nbytes / statistics.median(ts) / 1e3, 1)
        rec["dropout_over_copy"] = round(rec["dropout_us"] / rec["copy_cast_us"], 3)
        rec["inplace_over_copy"] = round(rec["dropout_inplace_us"] / rec["copy_cast_us"], 3)
        print(json.dumps(rec), flush=True)


def child_step(a):
    import torch
    import torch.nn.functional as F
    from kdcc_amd.models.cifar_models import wrn
    torch.manual_seed(0)
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    model = wrn(depth=28, widen_factor=10, num_classes=100, dropRate=a.rate).cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    x = torch.randn((a.batch, 3, 32, 32), device="cuda").to(dtype=dtype, memory_format=torch.channels_last)
    target = torch.randint(0, 100, (a.batch,), device="cuda")

    def step():
        loss = F.cross_entropy(model(x), target)
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
    print(json.dumps({"tool": "bench_dropout", "what": "step", "dtype": a.dtype, "dropRate": a.rate, "batch": a.batch, "steps": a.steps,
                      "ms_per_step": round(ms, 3), "img_per_s": round(a.batch * 1e3 / ms, 1), "loss": float(loss.detach())}), flush=True)


def tables(lines, a):
    med = lambda xs: statistics.median(xs)
    out = [f"`python tools/bench_dropout.py --rounds {a.rounds} --steps {a.steps} --warmup {a.warmup} --batch {a.batch}`: medians over the rounds; "
           "every line of the run is in the `.jsonl` beside this file.", "",
           "| dtype | shape (ld) | MB per call | `kd_copy_cast` us (GB/s) | `kd_dropout_nhwc` us (GB/s) | in place us (GB/s) | dropout / copy | in place / copy |",
           "|---|---|---|---|---|---|---|---|"]
    for dname in ("fp32", "bf16"):
        for shape in SHAPES:
            ks = [l for l in lines if l["what"] == "kernel" and l["dtype"] == dname and tuple(l["shape"]) == shape]
            if not ks:
                continue
            nb = ks[0]["bytes_per_call"]
            c, d, i = (med([k[n + "_us"] for k in ks]) for n in ("copy_cast", "dropout", "dropout_inplace"))
            cell = lambda us: f"{us:.1f} ({nb / us / 1e3:.0f})"
            out.append(f"| {dname} | {'x'.join(map(str, shape))} ({ks[0]['ld']}) | {nb / 1e6:.1f} | {cell(c)} | {cell(d)} | {cell(i)} | {d / c:.2f} | {i / c:.2f} |")
    out += ["", "| dtype | dropRate 0 ms per step | dropRate 0.3 ms per step | ratio | share of the step |", "|---|---|---|---|---|"]
    for dname in ("fp32", "bf16"):
        ss = {r: [l["ms_per_step"] for l in lines if l["what"] == "step" and l["dtype"] == dname and l["dropRate"] == r] for r in (0.0, 0.3)}
        if ss[0.0] and ss[0.3]:
            p, d = med(ss[0.0]), med(ss[0.3])
            out.append(f"| {dname} | {p:.2f} ({', '.join('%.2f' % v for v in ss[0.0])}) | {d:.2f} ({', '.join('%.2f' % v for v in ss[0.3])}) | {d / p:.3f} | "
                       f"{100 * (d - p) / d:.1f} % |")
    return "\n".join(out)


def write_markdown(path, body):
    text = f"# Dropout on HIP: the pass and what it costs a step\n\n{BEGIN}\n{END}\n"
    if os.path.exists(path):
        with open(path) as f:
            text = f.read()
    if BEGIN not in text or END not in text:
        text += f"\n{BEGIN}\n{END}\n"
    head, rest = text.split(BEGIN, 1)
    with open(path, "w") as f:
        f.write(head + BEGIN + "\n" + body + "\n" + END + rest.split(END, 1)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--kernel-bytes", type=float, default=4e11, help="bytes a timed block of the kernel child moves (sets its iterations)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout"), help="path without extension: <out>.jsonl and <out>.md")
    ap.add_argument("--child", choices=("kernel", "step"))
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--rate", type=float, default=0.0)
    ap.add_argument("--only", type=int, help="kernel child: the one (dtype, shape) to run, 0..5 in the table's order")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        import kdcc_amd  # noqa: F401
        child_kernel(a) if a.child == "kernel" else child_step(a)
        return 0
    lines = []
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch), "--kernel-bytes", str(a.kernel_bytes)]
    children = [["--child", "kernel"]] + [["--child", "step", "--dtype", d, "--rate", str(r)] for d in ("fp32", "bf16") for r in (0.0, 0.3)]
    for r in range(a.rounds):
        for child in children:
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + child + common, capture_output=True, text=True, timeout=a.child_timeout)
            if p.returncode != 0:
                print(f"child {child} (round {r}) exited {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
                return 1
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    rec = json.loads(ln)
                    rec["round"] = r
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".jsonl", "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    body = tables(lines, a)
    write_markdown(a.out + ".md", body)
    print(body)
    return 0


if __name__ == "__main__":
    sys.exit(main())
