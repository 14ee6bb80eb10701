#!/usr/bin/env python3
"""Timing only (not on the test path): the criteria kernels at the headline logit shape, 8 x 19 x 1024 x 2048 fp32 channels-last,
each next to the existing kernel that moves the same bytes, in one process -- kd_jsdiv / kd_ensemble_kldiv vs kd_kldiv (fwd + grad),
kd_jsdiv_up vs kd_kldiv_up and kd_focal_up vs kd_ce2d_up (from the 8 x 512 x 1024 x 19 half-resolution logits), kd_focal +
kd_focal_grad vs kd_ce2d + kd_ce2d_grad -- and kd_topk_hint_mse on a 4096-channel 128 x 256 hint.

    python tools/bench_criteria.py [--iters 20] [--warmup 3]

Prints one JSON line per kernel (median / min ms over the timed calls, effective GB/s of the algorithmic bytes) and the ratios
the criteria are held to."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timeit(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from kdcc_amd import ops
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    N, Cc, H, W = 8, 19, 1024, 2048
    cl = torch.channels_last
    s = (torch.randn((N, Cc, H, W), device="cuda", generator=gen) * 3).contiguous(memory_format=cl)
    t = (torch.randn((N, Cc, H, W), device="cuda", generator=gen) * 3).contiguous(memory_format=cl)
    pt = torch.softmax(t, 1).contiguous(memory_format=cl)
    tgt = torch.randint(0, Cc, (N, H, W), device="cuda", generator=gen)
    tgt[:, :64] = 255
    s_lo = torch.randn((N, H // 2, W // 2, Cc), device="cuda", generator=gen) * 3
    t_lo = torch.randn((N, H // 2, W // 2, Cc), device="cuda", generator=gen) * 3
    one = torch.ones((), device="cuda")
    full = s.numel() * 4
    lo = s_lo.numel() * 4
    lbl = tgt.numel() * 8

    def focal_fwd_grad():
        _, st, _, _ = ops.focal(s, tgt, 2.0, None, 255, "mean")
        ops.focal_grad(s, tgt, 2.0, None, 255, "mean", one, st)

    def ce_fwd_grad():
        ops.ce2d(s, tgt, 255)
        ops.ce2d_grad(s, tgt, 255)

    cases = [
        ("kd_kldiv fwd+grad", lambda: ops.kldiv(s, t, 4.0), 3 * full),
        ("kd_jsdiv fwd+grad", lambda: ops.jsdiv(s, t, 4.0), 3 * full),
        ("kd_ensemble_kldiv fwd+grad", lambda: ops.ensemble_kldiv(s, pt), 3 * full),
        ("kd_kldiv_up", lambda: ops.kldiv_up(s_lo, t_lo, (H, W), 4.0), 2 * lo),
        ("kd_jsdiv_up", lambda: ops.jsdiv_up(s_lo, t_lo, (H, W), 4.0), 2 * lo),
        ("kd_ce2d_up", lambda: ops.ce2d_up(s_lo, tgt, (H, W), 255), lo + lbl),
        ("kd_focal_up", lambda: ops.focal_up(s_lo, tgt, (H, W), 2.0, None, 255, "mean"), lo + lbl),
        ("kd_ce2d + kd_ce2d_grad", ce_fwd_grad, 3 * full + 2 * lbl),
        ("kd_focal + kd_focal_grad", focal_fwd_grad, 3 * full + 2 * lbl),
    ]
    res = {}
    for name, fn, nbytes in cases:
        med, mn = timeit(fn, a.iters, a.warmup)
        res[name] = med
        print(json.dumps({"kernel": name, "shape": [N, Cc, H, W], "median_ms": round(med, 4), "min_ms": round(mn, 4),
                          "GBps": round(nbytes / med / 1e6, 1)}), flush=True)
    del s, t, pt, s_lo, t_lo
    hs = torch.randn((N, 4096, 128, 256), device="cuda", generator=gen).contiguous(memory_format=cl)
    ht = torch.randn((N, 4096, 128, 256), device="cuda", generator=gen).contiguous(memory_format=cl)
    for name, fn, nbytes in (("kd_hint_mse fwd+grad (4096ch)", lambda: ops.hint_mse(hs, ht, 1.0), 3 * hs.numel() * 4),
                             ("kd_topk_hint_mse fwd+grad (4096ch)", lambda: ops.topk_hint_mse(hs, ht, 2048), 5 * hs.numel() * 4)):
        med, mn = timeit(fn, a.iters, a.warmup)
        res[name] = med
        print(json.dumps({"kernel": name, "shape": list(hs.shape), "median_ms": round(med, 4), "min_ms": round(mn, 4),
                          "GBps": round(nbytes / med / 1e6, 1)}), flush=True)
    print(json.dumps({"ratios": {
        "jsdiv/kldiv": round(res["kd_jsdiv fwd+grad"] / res["kd_kldiv fwd+grad"], 3),
        "ensemble_kldiv/kldiv": round(res["kd_ensemble_kldiv fwd+grad"] / res["kd_kldiv fwd+grad"], 3),
        "jsdiv_up/kldiv_up": round(res["kd_jsdiv_up"] / res["kd_kldiv_up"], 3),
        "focal_up/ce2d_up": round(res["kd_focal_up"] / res["kd_ce2d_up"], 3),
        "focal+grad/ce2d+grad": round(res["kd_focal + kd_focal_grad"] / res["kd_ce2d + kd_ce2d_grad"], 3),
        "topk/hint_mse": round(res["kd_topk_hint_mse fwd+grad (4096ch)"] / res["kd_hint_mse fwd+grad (4096ch)"], 3)}}))


if __name__ == "__main__":
    main()
