#!/usr/bin/env python3
"""Generate tests/golden/criteria.npz and tests/golden/criteria_names.json from the REFERENCE's own criteria (CPU, fp32).

Runs only in the build container, like tools/make_golden.py (it imports the reference, which does not exist on the GPU box and
must never travel).  Only data is written: seeded inputs, the reference's losses and autograd gradients, and the names and
constructor signatures of its `losses` package.

    cd /path/to/reference && python3 /path/to/repo/tools/make_golden_criteria.py

Covers JSDivergenceLoss (T in {1, 4}, 4-D and (N,C)), EnsembleKLDivergenceLoss, FocalLoss (gamma x reduction x alpha x
ignore_index, ignored pixels present; 'none' back-propagates a seeded upstream gradient) and TopkHintMSELoss (topk in
{0.5, 0.25}, C in {24, 64}, target norms well separated at the pivot).
"""
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("KD_REFERENCE", "/root/reference")
os.chdir(REF)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

torch.Tensor.cuda = lambda self, *a, **k: self          # TopkHintMSELoss moves its mask with .cuda()

import warnings
warnings.filterwarnings("ignore")

import losses as ref_losses                              # noqa: E402

from _seeded import seeded_input                         # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")


def run(out, tag, crit, s, t, upstream=None):
    s = s.clone().requires_grad_(True)
    loss = crit(s, t)
    if upstream is None:
        loss.backward()
    else:
        loss.backward(upstream)
        out[f"{tag}.up"] = upstream.numpy()
    out[f"{tag}.s"] = s.detach().numpy()
    out[f"{tag}.loss"] = loss.detach().numpy().astype(np.float32) if loss.dim() else np.float64(loss.item())
    out[f"{tag}.grad"] = s.grad.numpy()


def g_criteria():
    out = {}
    # JSD: (N,C,H,W) and (N,C); targets are constants
    s4, t4 = seeded_input("crit.s4", (2, 19, 8, 16)) * 2, seeded_input("crit.t4", (2, 19, 8, 16)) * 2
    s2, t2 = seeded_input("crit.s2", (32, 10), 2.0), seeded_input("crit.t2", (32, 10), 2.0)
    for T in (1, 4):
        run(out, f"jsd_T{T}", ref_losses.JSDivergenceLoss(T), s4, t4)
        out[f"jsd_T{T}.t"] = t4.numpy()
        run(out, f"jsd2d_T{T}", ref_losses.JSDivergenceLoss(T), s2, t2)
        out[f"jsd2d_T{T}.t"] = t2.numpy()
    # ensemble KL: soft targets with exact zeros (xlogy: 0 log 0 = 0)
    p = torch.softmax(seeded_input("crit.ekl_t", (2, 19, 8, 16)) * 2, 1)
    p[:, 3] = 0.0
    p[0, 7, :2] = 0.0
    p = p / p.sum(1, keepdim=True)
    run(out, "ekl", ref_losses.EnsembleKLDivergenceLoss(), s4, p)
    out["ekl.t"] = p.numpy()
    # focal: gamma x reduction x alpha x ignore_index
    C = 7
    xf = seeded_input("crit.focal_x", (2, C, 6, 8)) * 2
    alpha = torch.rand(C, generator=torch.Generator().manual_seed(11)) + 0.5
    out["focal.x"] = xf.numpy()
    out["focal.alpha"] = alpha.numpy()
    for ign in (-100, 255):
        tgt = torch.randint(0, C, (2, 6, 8), generator=torch.Generator().manual_seed(12))
        tgt[:, 0] = ign
        tgt[1, 3, 2:5] = ign
        out[f"focal.target_{'m100' if ign < 0 else ign}"] = tgt.numpy()
        for gamma in (0, 2, 0.5):
            for red in ("none", "mean", "sum"):
                for an, a in (("noalpha", None), ("alpha", alpha)):
                    tag = f"focal_g{gamma}_{red}_{an}_{'m100' if ign < 0 else ign}"
                    up = None
                    if red == "none":
                        up = torch.randn((2, 2, 6, 8), generator=torch.Generator().manual_seed(13))
                    run(out, tag, ref_losses.FocalLoss(gamma, alpha=a, ignore_index=ign, reduction=red), xf, tgt, up)
                    del out[f"{tag}.s"]          # (= focal.x)
    # top-k hint: per-sample channel scales 1 + 0.1 * (a permutation): neighbouring norms at the pivot differ by >= 1.5 %
    for Cc in (24, 64):
        hs = seeded_input(f"crit.topk_s{Cc}", (2, Cc, 6, 8))
        base = seeded_input(f"crit.topk_t{Cc}", (2, Cc, 6, 8))
        base = base / base.norm(dim=(-1, -2), keepdim=True)
        perm = torch.stack([torch.randperm(Cc, generator=torch.Generator().manual_seed(20 + Cc + n)) for n in range(2)])
        ht = base * (1.0 + 0.1 * perm.float())[:, :, None, None]
        for k in (0.5, 0.25):
            tag = f"topk_{Cc}_{k}"
            run(out, tag, ref_losses.TopkHintMSELoss(topk=k), hs, ht)
            out[f"{tag}.t"] = ht.numpy()
    path = os.path.join(OUT, "criteria.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays)")


def g_names():
    """Every class the reference's losses package exports, with its constructor parameters and defaults (data only)."""
    inv = {}
    for name in sorted(dir(ref_losses)):
        obj = getattr(ref_losses, name)
        if not (inspect.isclass(obj) and issubclass(obj, torch.nn.Module)):
            continue
        params = []
        for pn, prm in inspect.signature(obj.__init__).parameters.items():
            if pn == "self":
                continue
            params.append({"name": pn, "required": prm.default is inspect.Parameter.empty,
                           "default": None if prm.default is inspect.Parameter.empty else prm.default})
        inv[name] = params
    path = os.path.join(OUT, "criteria_names.json")
    with open(path, "w") as f:
        json.dump(inv, f, indent=1, sort_keys=True)
    print("wrote", path, sorted(inv))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    g_criteria()
    g_names()
