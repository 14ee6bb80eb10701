#!/usr/bin/env python3
"""Achieved bytes/s of the NHWC BatchNorm entry points on the Wide-ResNet-28-10 shapes at batch 128, fp32 (kd_bn_nhwc_fwd / _bwd)
next to bf16 (kd_bn_nhwc_lp_fwd / _bwd): train mode, fused ReLU, the backward with `res`, dgamma and dbeta.

    python tools/bench_bn_nhwc.py [--iters 50] [--warmup 5]

Time: HIP events around `iters` calls (each call is all of its launches: two reduction stages and the elementwise pass).  Bytes: what
the algorithm has to move, from the shapes -- forward: x read twice (statistics, normalise) and y written once = 3 M C e; backward: gy,
x and y read by the reduction and again by the dx pass, res read and dx written = 8 M C e (e = 4 or 2 bytes; the per-channel
vectors and the partial sums are left out).  Prints one JSON line per shape and dtype."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(128, 32, 32, 160), (128, 16, 16, 320), (128, 8, 8, 640)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    torch.manual_seed(0)
    for shape in SHAPES:
        N, H, W, C = shape
        M = N * H * W
        gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
        for dtype in (torch.float32, torch.bfloat16):
            x, gy, res = (torch.randn(shape, device="cuda").to(dtype) for _ in range(3))
            rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
            y, mean, invstd = ops.bn_nhwc_fwd(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True)
            dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
            fwd = timed(lambda: ops.bn_nhwc_fwd(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True, out=y), a.iters, a.warmup)
            dx = torch.empty_like(x)
            bwd = timed(lambda: ops.bn_nhwc_bwd(gy, x, y, gamma, mean, invstd, True, True, res=res, dgamma=dg, dbeta=db, out=dx), a.iters, a.warmup)
            e = x.element_size()
            print(json.dumps({"tool": "bench_bn_nhwc", "shape": list(shape), "dtype": str(dtype).split(".")[1],
                              "fwd_us": round(fwd * 1e3, 1), "fwd_GBps": round(3 * M * C * e / fwd / 1e6, 1),
                              "bwd_us": round(bwd * 1e3, 1), "bwd_GBps": round(8 * M * C * e / bwd / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
