#!/usr/bin/env python3
"""Timing only (not on the test path): the HRNet-OCR kernels against the compositions they replace, and one LayerwiseTrainer step,
all at the shapes of cfg/cityscapes/10M_hrnet_all.json -- crop 512, batch 4, HRNetV2-W48: branch maps 128 / 64 / 32 / 16, OCR
HW = 16384, 19 classes, 512 mid / 256 key channels.

  * fuse sum (stage-4 exchange unit onto the 48-channel 128x128 branch, four sources), forward and backward: kd_hr_fuse_fwd / _bwd
    against kd_upsample_bilinear_ac (+ _bwd) per coarser source, torch adds and ReLU;
  * OCR spatial gather and object attention, forward and backward: kd_ocr_gather_* / kd_ocr_attend_* against torch softmax + matmul
    (autograd for the backward);
  * one whole LayerwiseTrainer step (teacher forward, student forward, hint loss, backward, RAdam) with the shipped plan applied to
    randomly initialised W48 weights.

    python tools/bench_hrnet.py [--iters 20] [--warmup 3] [--steps 5] [--skip-step] [--out profiles/hrnet_ocr.md]

One process, the project's usual warm-up and median (tools/bench_criteria.py timeit).  Prints one JSON line per measurement and
writes the table to --out.  Nothing is asserted: a kernel that loses to its composition is reported as such."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_criteria import timeit  # noqa: E402

N, CROP, K, MID, KEY = 4, 512, 19, 512, 256
ROWS = []


def report(case, new_ms, old_ms, nbytes=None, note=""):
    row = {"tool": "bench_hrnet", "case": case, "kernel_ms": round(new_ms, 4), "composition_ms": round(old_ms, 4),
           "speedup": round(old_ms / new_ms, 2)}
    if nbytes:
        row["kernel_GBps"] = round(nbytes / new_ms / 1e6, 1)
    print(json.dumps(row), flush=True)
    ROWS.append((case, new_ms, old_ms, row.get("kernel_GBps"), note))


def bench_fuse(a):
    from kdcc_amd import ops
    C, sizes = 48, [(128, 128), (64, 64), (32, 32), (16, 16)]
    srcs = [torch.randn(N, h, w, C, device="cuda") for h, w in sizes]
    gy = torch.randn(N, 128, 128, C, device="cuda")

    def composed_fwd():
        y = srcs[0]
        for s in srcs[1:]:
            y = y + ops.upsample_bilinear_ac(s, sizes[0])
        return torch.relu(y)

    y = ops.hr_fuse(srcs)
    assert float((y - composed_fwd()).abs().max()) < 1e-4

    def composed_bwd():
        g = gy * (y > 0)
        return [g] + [ops.upsample_bilinear_ac_bwd(g, s) for s in sizes[1:]]

    big = y.numel() * 4
    small = sum(s.numel() for s in srcs[1:]) * 4
    report("fuse_fwd 4 sources 48ch 128x128", timeit(lambda: ops.hr_fuse(srcs), a.iters, a.warmup)[0], timeit(composed_fwd, a.iters, a.warmup)[0],
           2 * big + small)
    report("fuse_bwd 4 sources 48ch 128x128", timeit(lambda: ops.hr_fuse_bwd(gy, y, sizes), a.iters, a.warmup)[0],
           timeit(composed_bwd, a.iters, a.warmup)[0], 3 * big + small)


def bench_gather(a):
    from kdcc_amd import ops
    HW = (CROP // 4) ** 2
    logits, feats = torch.randn(N, HW, K, device="cuda") * 3, torch.randn(N, HW, MID, device="cuda")
    gctx = torch.randn(N, K, MID, device="cuda")
    lt, ft = logits.clone().requires_grad_(True), feats.clone().requires_grad_(True)

    def composed_fwd():
        return torch.matmul(F.softmax(lt, dim=1).transpose(1, 2), ft)

    def composed_fwd_bwd():
        lt.grad = ft.grad = None
        composed_fwd().backward(gctx)

    ctx, _, lse = ops.ocr_gather(logits, feats)
    assert float((ctx - composed_fwd().detach()).abs().max()) < 1e-3
    fwd_old = timeit(lambda: composed_fwd().detach(), a.iters, a.warmup)[0]
    report("ocr_gather_fwd HW=16384 K=19 C=512", timeit(lambda: ops.ocr_gather(logits, feats), a.iters, a.warmup)[0], fwd_old, feats.numel() * 4)
    both_old = timeit(composed_fwd_bwd, a.iters, a.warmup)[0]
    report("ocr_gather_bwd HW=16384 K=19 C=512", timeit(lambda: ops.ocr_gather_bwd(gctx, ctx, logits, feats, lse), a.iters, a.warmup)[0],
           max(both_old - fwd_old, 1e-6), 2 * feats.numel() * 4, "composition = (forward + backward) - forward of torch autograd")


def bench_attend(a):
    from kdcc_amd import ops
    HW = (CROP // 4) ** 2
    q, k, v = torch.randn(N, HW, KEY, device="cuda"), torch.randn(N, K, KEY, device="cuda"), torch.randn(N, K, KEY, device="cuda")
    g = torch.randn(N, HW, KEY, device="cuda")
    qt, kt, vt = (t.clone().requires_grad_(True) for t in (q, k, v))

    def composed_fwd():
        return torch.matmul(F.softmax(torch.matmul(qt, kt.transpose(1, 2)) * KEY ** -0.5, dim=-1), vt)

    def composed_fwd_bwd():
        qt.grad = kt.grad = vt.grad = None
        composed_fwd().backward(g)

    assert float((ops.ocr_attend(q, k, v) - composed_fwd().detach()).abs().max()) < 1e-3
    fwd_old = timeit(lambda: composed_fwd().detach(), a.iters, a.warmup)[0]
    report("ocr_attend_fwd HW=16384 K=19 Ck=256", timeit(lambda: ops.ocr_attend(q, k, v), a.iters, a.warmup)[0], fwd_old, 2 * q.numel() * 4)
    both_old = timeit(composed_fwd_bwd, a.iters, a.warmup)[0]
    report("ocr_attend_bwd HW=16384 K=19 Ck=256", timeit(lambda: ops.ocr_attend_bwd(g, q, k, v), a.iters, a.warmup)[0],
           max(both_old - fwd_old, 1e-6), 5 * q.numel() * 4, "composition = (forward + backward) - forward of torch autograd; the kernel reads q and g twice")


def bench_step(a):
    from kdcc_amd import losses, models
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.utils.optim import RAdam
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg", "cityscapes", "10M_hrnet_all.json")))
    torch.manual_seed(0)
    teacher = models.HighResolutionNet(**cfg["teacher"]["args"]).cuda().eval()
    model = DepthwiseStudent(teacher, None)
    pr = cfg["pruning"]
    model.replace(pr["pruning_plan"], **pr["args"])
    model.register_hint_layers([e["name"] for e in pr["hint"]])
    model.unfreeze([e["name"] for e in pr["unfreeze"]])
    model.student.eval()
    crit = losses.MSELoss(**cfg["hint_loss"]["args"])
    opt = RAdam([p for p in model.student.parameters() if p.requires_grad], **cfg["optimizer"]["args"])
    x = torch.randn(N, 3, CROP, CROP, device="cuda")

    def step():
        model(x)
        loss = sum(crit(s, t) for s, t in zip(model.student_hidden_outputs, model.teacher_hidden_outputs))
        loss.backward()
        opt.step()
        opt.zero_grad()

    ms = timeit(step, a.steps, a.warmup)[0]
    print(json.dumps({"tool": "bench_hrnet", "case": "layerwise_step W48 batch 4 crop 512", "ms_per_step": round(ms, 2),
                      "img_per_s": round(N * 1e3 / ms, 2)}), flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hrnet_ocr.md"))
    a = ap.parse_args()
    import kdcc_amd  # noqa: F401
    torch.cuda.set_device(0)
    bench_fuse(a)
    bench_gather(a)
    bench_attend(a)
    step_ms = None if a.skip_step else bench_step(a)
    lines = ["# HRNet-OCR kernels at the shipped config's shapes", "",
             "`python tools/bench_hrnet.py` on one MI355X: batch 4, crop 512, HRNetV2-W48 (branch maps 128 / 64 / 32 / 16, OCR HW = 16384,",
             f"19 classes), fp32; median of {a.iters} timed calls after {a.warmup} warm-up calls, one process.", "",
             "| case | kernel ms | composition ms | composition / kernel | kernel GB/s (algorithmic bytes) |", "|---|---|---|---|---|"]
    for case, new, old, gbps, note in ROWS:
        lines.append(f"| {case} | {new:.4f} | {old:.4f} | {old / new:.2f} | {gbps if gbps else ''} |")
    notes = [f"- {case}: {note}" for case, _, _, _, note in ROWS if note]
    if notes:
        lines += ["", *notes]
    losers = [case for case, new, old, _, _ in ROWS if new > old]
    lines += ["", "Kernels slower than the composition they replace at these shapes: " + (", ".join(losers) if losers else "none") + "."]
    if step_ms is not None:
        lines += ["", f"One LayerwiseTrainer step (teacher forward, student forward, 8 hint losses, backward, RAdam; randomly initialised "
                      f"weights): {step_ms:.1f} ms, {N * 1e3 / step_ms:.2f} img/s (median of {a.steps})."]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
