#!/usr/bin/env python3
"""Timing only (not on the test path): the layer-compressibility analysis step (AnalysisStudent / AnalysisTrainer).

At batch 4, 512 x 512, bf16, for mod4.block2.convs.conv2, aspp.features.1.0 and mod7.block1.convs.conv3 (droprate 0.85):
  * the analysis step: forward of teacher and probed student, the step's logged metrics, hint loss, backward, RAdam;
  * the masked site's forward (frozen conv on the kept filters -> compact tensor -> 1x1 on Kp input channels) against the same
    site run uncompacted from existing ops: the full frozen conv, the mask multiply, the full 1x1;
  * the fused metrics call (ops.logit_metrics_up) against the composition it replaces: materialise both logit tensors, two
    ce2d, hint_mse, two confusion.
The metrics pair is also timed at the bench's 8 x 1024 x 2048.  Every comparison runs both sides alternately, five repeats each,
and reports the medians and the min-max spread between repeats; run the tool in a fresh process per measurement session.

    python tools/bench_analysis.py [--iters 20] [--warmup 5] [--steps 8] [--out profiles/analysis_step.md]

Prints one JSON line per measurement and writes the table to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_criteria import timeit  # noqa: E402

LAYERS = ["mod4.block2.convs.conv2", "aspp.features.1.0", "mod7.block1.convs.conv3"]


def ab(fa, fb, a):
    """(medians a, medians b) of five alternating repeats."""
    ra, rb = [], []
    for _ in range(5):
        ra.append(timeit(fa, a.iters, a.warmup)[0])
        rb.append(timeit(fb, a.iters, a.warmup)[0])
    return ra, rb


def stats(v):
    return {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def metrics_case(name, N, h, w, H, W, a, rows):
    from kdcc_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(0)
    s_lo = torch.randn((N, h, w, 19), device="cuda", generator=gen) * 3
    t_lo = s_lo + torch.randn((N, h, w, 19), device="cuda", generator=gen)
    tgt = torch.randint(0, 19, (N, H, W), device="cuda", generator=gen)
    tgt[:, :8] = 255
    cs, ct = torch.zeros((19, 19), dtype=torch.int64, device="cuda"), torch.zeros((19, 19), dtype=torch.int64, device="cuda")

    def fused():
        ops.logit_metrics_up(s_lo, t_lo, tgt, (H, W), 255, True, conf_s=cs, conf_t=ct, accumulate=True)

    def composed():
        S = ops.upsample_bilinear_ac(s_lo, (H, W), out_dtype=torch.float32).permute(0, 3, 1, 2)
        T = ops.upsample_bilinear_ac(t_lo, (H, W), out_dtype=torch.float32).permute(0, 3, 1, 2)
        ops.ce2d(S, tgt, 255); ops.ce2d(T, tgt, 255)
        ops.hint_mse(S, T, 1.0, want_grad=False)
        ops.confusion(S, tgt, cs, accumulate=True); ops.confusion(T, tgt, ct, accumulate=True)
    # both sides compute the same numbers at the timed size before anything is timed
    o, fs, ft = ops.logit_metrics_up(s_lo, t_lo, tgt, (H, W), 255, True)
    S = ops.upsample_bilinear_ac(s_lo, (H, W), out_dtype=torch.float32).permute(0, 3, 1, 2)
    T = ops.upsample_bilinear_ac(t_lo, (H, W), out_dtype=torch.float32).permute(0, 3, 1, 2)
    ref = torch.stack([ops.ce2d(S, tgt, 255), ops.ce2d(T, tgt, 255), ops.hint_mse(S, T, 1.0, want_grad=False)[0]])
    same = bool(torch.equal(fs, ops.confusion(S, tgt)) and torch.equal(ft, ops.confusion(T, tgt)))
    rel = float(((o - ref).abs() / ref.abs().clamp_min(1e-30)).max())
    del S, T
    cs.zero_(); ct.zero_()
    rf, rc = ab(fused, composed, a)
    rec = {"tool": "bench_analysis", "case": "metrics " + name, "shape": [N, 19, H, W], "fused": stats(rf), "composed": stats(rc),
           "confusion_equal": same, "float_outputs_max_rel_diff": rel, "composed_spread_ms": round(max(rc) - min(rc), 4)}
    rec["speedup"] = round(rec["composed"]["median_ms"] / rec["fused"]["median_ms"], 2)
    rec["not_slower"] = rec["fused"]["median_ms"] <= rec["composed"]["median_ms"] + (max(rc) - min(rc))
    print(json.dumps(rec), flush=True)
    rows.append(rec)


def site_case(name, model, x, a, rows):
    """The masked site alone, on its own input taken from the engine's tape."""
    from kdcc_amd import ops
    from kdcc_amd._lib import KD_PACK_FWD
    eng = model._student_engine()
    eng.hint_names = [name]
    with torch.no_grad():
        eng.forward(x)
    blk = model.get_block(name, model.student)
    if name.startswith("aspp"):
        a_in, site = eng._tape["aspp"]["x7"], [b["site"] for b in eng._tape["aspp"]["branches"] if b["site"].name == name][0]
    else:
        rec = [r for r in eng._tape["blocks"] if r is not None and r["name"] == name.split(".convs.")[0]][0]
        si = [s.name for s in rec["sites"]].index(name)
        a_in, site = rec["a_in"][si], rec["sites"][si]
    eng._tape = None
    conv, pw = blk[0], blk[2]
    N, H, W, _ = a_in.shape
    C = pw.out_channels
    _, kk, kp = eng._keep(site)
    out = torch.empty((N, H, W, C), dtype=a_in.dtype, device="cuda")
    w_full, w_pw = ops.pack_conv_weight(conv.weight, a_in.dtype, KD_PACK_FWD), ops.pack_conv_weight(pw.weight, a_in.dtype, KD_PACK_FWD)
    full = torch.empty((N, H, W, C), dtype=a_in.dtype, device="cuda")
    mask = blk[1].mask.reshape(1, 1, 1, -1).to(a_in.dtype)

    def masked():
        eng._masked_fwd(site, a_in, out_raw=out)

    def uncompacted():
        ops.conv2d(a_in, w_full, site.stride, site.pad, site.dil, out_raw=full)
        ops.conv2d(full * mask, w_pw, out_raw=out)
    masked(); got = out.float().clone()
    uncompacted(); want = out.float()
    rel = float((got - want).norm() / want.norm().clamp_min(1e-30))
    rm, ru = ab(masked, uncompacted, a)
    r = {"tool": "bench_analysis", "case": "site " + name, "input": [N, H, W, site.cin], "C": C, "kept": kk, "Kp": kp, "k": site.k,
         "masked": stats(rm), "uncompacted": stats(ru), "outputs_rel_l2_diff": rel, "uncompacted_spread_ms": round(max(ru) - min(ru), 4)}
    r["speedup"] = round(r["uncompacted"]["median_ms"] / r["masked"]["median_ms"], 2)
    print(json.dumps(r), flush=True)
    rows.append(r)


def step_case(name, model, x, tgt, a, rows):
    from kdcc_amd import losses
    from kdcc_amd.utils import CityscapesMetricTracker
    from kdcc_amd.utils.optim import RAdam
    from kdcc_amd import ops
    blk = model.get_block(name, model.student)
    opt = RAdam([blk[2].weight], lr=1e-3)
    hint_c = losses.MSELoss("mean", 1000)
    trk = (CityscapesMetricTracker(), CityscapesMetricTracker())

    def step():
        st, tc = model(x)
        o, cs, ct = ops.logit_metrics_up(st.low, tc.low, tgt, st.size_hw, 255, st.align_corners)
        trk[0].add_confusion(cs); trk[1].add_confusion(ct)
        loss = sum(hint_c(s, t) for s, t in zip(model.student_hidden_outputs, model.teacher_hidden_outputs))
        loss.backward()
        opt.step(); opt.zero_grad()
    reps = [timeit(step, a.steps, 3)[0] for _ in range(3)]
    r = {"tool": "bench_analysis", "case": "step " + name, "batch": x.shape[0], "crop": list(x.shape[2:]), "step": stats(reps),
         "img_per_s": round(x.shape[0] * 1e3 / sorted(reps)[1], 1)}
    print(json.dumps(r), flush=True)
    rows.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analysis_step.md"))
    a = ap.parse_args()
    import kdcc_amd  # noqa: F401
    from kdcc_amd.models import DeepWV3Plus
    from kdcc_amd.models.students import AnalysisStudent
    torch.cuda.set_device(0)
    rows = []
    metrics_case("config shape (batch 4, 512x512)", 4, 256, 256, 512, 512, a, rows)
    if not a.skip_big:
        metrics_case("bench shape (8 x 1024x2048)", 8, 512, 1024, 1024, 2048, a, rows)
    torch.manual_seed(0)
    np.random.seed(0)
    teacher = DeepWV3Plus(num_classes=19).eval()
    model = AnalysisStudent(teacher, None, dtype=torch.bfloat16).cuda()
    x = torch.randn((4, 3, 512, 512), device="cuda")
    tgt = torch.randint(0, 19, (4, 512, 512), device="cuda")
    for name in LAYERS:
        model.replace([name], droprate=0.85)
        model.register_hint_layers([name])
        site_case(name, model, x, a, rows)
        step_case(name, model, x, tgt, a, rows)
        model.reset()
    lines = ["# Layer-compressibility analysis step (tools/bench_analysis.py)", "",
             f"MI355X, bf16, batch 4, 512x512 crop, droprate 0.85; medians of {a.iters} timed calls after {a.warmup} warm-up calls, five",
             "alternating repeats per side (three for the whole step), `min..max` is the spread between repeats.", "",
             "Both sides of a comparison are run on the same tensors and their outputs compared at the timed size first.", "",
             "| measurement | code under test (ms) | composition of existing ops (ms) | ratio | same outputs | verdict |",
             "|---|---|---|---|---|---|"]
    fmt = lambda s: f"{s['median_ms']:.3f} ({s['min_ms']:.3f}..{s['max_ms']:.3f})"
    for r in rows:
        if r["case"].startswith("metrics"):
            lines.append(f"| {r['case']}: logit_metrics_up vs materialise + 2 ce2d + hint_mse + 2 confusion | {fmt(r['fused'])} | {fmt(r['composed'])} | "
                         f"{r['speedup']}x | confusion matrices equal: {r['confusion_equal']}; floats within {r['float_outputs_max_rel_diff']:.1e} | "
                         f"{'not slower' if r['not_slower'] else 'SLOWER'} than the composition's median + its spread ({r['composed_spread_ms']:.3f} ms) |")
        elif r["case"].startswith("site"):
            lines.append(f"| {r['case']} forward ({r['k']}x{r['k']}, C {r['C']}, kept {r['kept']}, Kp {r['Kp']}) vs full conv + mask + full 1x1 | "
                         f"{fmt(r['masked'])} | {fmt(r['uncompacted'])} | {r['speedup']}x | relative L2 difference {r['outputs_rel_l2_diff']:.1e} | "
                         f"spread of the composition {r['uncompacted_spread_ms']:.3f} ms |")
        else:
            lines.append(f"| {r['case']}: whole analysis step, {r['img_per_s']} img/s | {fmt(r['step'])} | - | - | - | - |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
