#!/usr/bin/env python3
"""Generate tests/golden/optim.npz by running the REFERENCE's optimizers themselves (CPU, fp32).

    KD_REFERENCE=<checkout of the reference> python3 tools/make_golden_optim.py

Like tools/make_golden.py: the reference's utils/optim/radam.py is imported (by file path: nothing else of the reference is
needed), only data -- seeded inputs and the parameters it produced -- is written, no reference source is copied.  Three runs
of 8 steps each on one 64-element tensor:
  plain      PlainRAdam(lr=0.005, weight_decay=1e-2): crosses N_sma >= 5 at step 6
  plain_nosgd  the same with degenerated_to_sgd=False: no parameter update before step 6
  adamw      AdamW(lr=0.005, warmup=4, weight_decay=1e-2): crosses the warm-up boundary at step 4
Each stores p (9, 64): the parameters before the first and after every step, and g (8, 64): the gradients."""
import importlib.util
import os
import sys
import warnings

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

from _seeded import seeded_input   # noqa: E402

warnings.filterwarnings("ignore")
STEPS, N, LR, WD, WARMUP = 8, 64, 0.005, 1e-2, 4


def reference_radam():
    ref = os.environ.get("KD_REFERENCE")
    if not ref:
        sys.exit("set KD_REFERENCE to a checkout of the reference")
    spec = importlib.util.spec_from_file_location("ref_radam", os.path.join(ref, "utils", "optim", "radam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(tag, make):
    p = seeded_input(f"optim.{tag}.p", (N,)).requires_grad_(True)
    opt = make([p])
    ps, gs = [p.detach().clone().numpy()], []
    for i in range(STEPS):
        g = seeded_input(f"optim.{tag}.g{i}", (N,))
        p.grad = g.clone()
        opt.step()
        gs.append(g.numpy())
        ps.append(p.detach().clone().numpy())
    return {f"{tag}.p": np.stack(ps), f"{tag}.g": np.stack(gs)}


def main():
    R = reference_radam()
    out = dict(lr=np.float64(LR), weight_decay=np.float64(WD), warmup=np.int64(WARMUP))
    out.update(run("plain", lambda ps: R.PlainRAdam(ps, lr=LR, weight_decay=WD)))
    out.update(run("plain_nosgd", lambda ps: R.PlainRAdam(ps, lr=LR, weight_decay=WD, degenerated_to_sgd=False)))
    out.update(run("adamw", lambda ps: R.AdamW(ps, lr=LR, warmup=WARMUP, weight_decay=WD)))
    assert np.array_equal(out["plain_nosgd.p"][0], out["plain_nosgd.p"][5]) and not np.array_equal(out["plain_nosgd.p"][5], out["plain_nosgd.p"][6])
    path = os.path.join(REPO, "tests", "golden", "optim.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
