"""The optimizer rules of csrc/optim.hip (kd_optim_step_multi) as a case table, and a float64 numpy restatement of them plus
PlainRAdam, written from the arithmetic include/kdcc.h states (torch.optim's single-tensor path; the reference's radam.py).

No GPU, no torch: test_optim_host.py holds the restatement to torch.optim run in float64, test_optim_gpu.py holds the kernels
to the restatement."""
import math

import numpy as np

OPT_BLK = 256 * 16                     # "constexpr int OPT_BLK = 256 * 16;" (csrc/optim.hip): elements per block
MAXT = {"sgd": 72, "adam": 48, "adamw_ref": 53}   # tensors per launch (OptBatch<>::MAXT; include/kdcc.h states them)
STEPS = 20

# every flag of every rule: (id, rule, constructor arguments)
CASES = [
    ("sgd-plain", "sgd", dict(lr=0.05)),
    ("sgd-wd", "sgd", dict(lr=0.05, weight_decay=5e-3)),
    ("sgd-momentum", "sgd", dict(lr=0.05, momentum=0.9)),
    ("sgd-momentum-dampening", "sgd", dict(lr=0.05, momentum=0.9, dampening=0.3)),
    ("sgd-nesterov-wd", "sgd", dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=5e-3)),
    ("sgd-maximize", "sgd", dict(lr=0.05, momentum=0.8, maximize=True)),
    ("adam-plain", "adam", dict(lr=0.01)),
    ("adam-wd", "adam", dict(lr=0.01, weight_decay=5e-3)),
    ("adam-amsgrad", "adam", dict(lr=0.01, amsgrad=True)),
    ("adam-amsgrad-wd", "adam", dict(lr=0.01, amsgrad=True, weight_decay=5e-3, betas=(0.8, 0.99))),
    ("adam-maximize", "adam", dict(lr=0.01, maximize=True)),
    ("adamw-warmup0", "adamw_ref", dict(lr=0.01)),
    ("adamw-warmup7", "adamw_ref", dict(lr=0.01, warmup=7)),
    ("adamw-wd", "adamw_ref", dict(lr=0.01, warmup=7, weight_decay=1e-2)),
]
IDS = [c[0] for c in CASES]

# the smallest sizes at which each path of the kernel can go wrong: below one 16-byte access, a scalar tail, one element either
# side of a block, many blocks with a tail
SIZES = [1, 3, 4, 7, OPT_BLK - 1, OPT_BLK, OPT_BLK + 1, 300001]


def inputs(seed, sizes, steps=STEPS):
    """fp32 parameters and per-step gradients, fixed by the seed: ([p0], [[g of step s] per tensor])."""
    rng = np.random.default_rng(seed)
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    gs = [[(rng.standard_normal(n) * (0.5 + 0.25 * (s % 3))).astype(np.float32) for s in range(steps)] for n in sizes]
    return p0, gs


def rect(step, beta1, beta2, degenerated_to_sgd=True):
    """(N_sma, step_size) of RAdam / PlainRAdam; step_size < 0: no parameter update."""
    beta2_t = beta2 ** step
    n_max = 2 / (1 - beta2) - 1
    n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma >= 5:
        return n_sma, math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - beta1 ** step)
    return n_sma, (1.0 / (1 - beta1 ** step) if degenerated_to_sgd else -1.0)


def step64(rule, p, g, state, step, lr=1e-3, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False, maximize=False,
           betas=(0.9, 0.999), eps=1e-8, amsgrad=False, warmup=0, degenerated_to_sgd=True):
    """One step of `rule` ("sgd", "adam", "adamw_ref", "plain_radam") on float64 arrays; `state` is the tensor's dict, `step` its
    count after the increment.  Returns the new p; the state is updated in place."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    b1, b2 = betas
    if rule == "sgd":
        if maximize:
            g = -g
        if weight_decay != 0:
            g = g + weight_decay * p
        if momentum != 0:
            state["momentum_buffer"] = g.copy() if "momentum_buffer" not in state else momentum * state["momentum_buffer"] + (1 - dampening) * g
            g = g + momentum * state["momentum_buffer"] if nesterov else state["momentum_buffer"]
        return p - lr * g
    if not state:
        state.update(exp_avg=np.zeros_like(p), exp_avg_sq=np.zeros_like(p))
        if amsgrad:
            state["max_exp_avg_sq"] = np.zeros_like(p)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    if rule == "adam":
        if maximize:
            g = -g
        if weight_decay != 0:
            g = g + weight_decay * p
        state["exp_avg"] = state["exp_avg"] + (1 - b1) * (g - state["exp_avg"])
        state["exp_avg_sq"] = b2 * state["exp_avg_sq"] + (1 - b2) * g * g
        v = state["exp_avg_sq"]
        if amsgrad:
            v = state["max_exp_avg_sq"] = np.maximum(state["max_exp_avg_sq"], v)
        return p - (lr / bc1) * state["exp_avg"] / (np.sqrt(v) / math.sqrt(bc2) + eps)
    state["exp_avg_sq"] = b2 * state["exp_avg_sq"] + (1 - b2) * g * g
    state["exp_avg"] = b1 * state["exp_avg"] + (1 - b1) * g
    if rule == "adamw_ref":
        slr = 1e-8 + step * lr / warmup if warmup > step else lr
        if weight_decay != 0:
            p = p + -weight_decay * slr * p
        return p + -(slr * math.sqrt(bc2) / bc1) * state["exp_avg"] / (np.sqrt(state["exp_avg_sq"]) + eps)
    assert rule == "plain_radam"
    n_sma, step_size = rect(step, b1, b2, degenerated_to_sgd)
    if step_size < 0:
        return p
    if weight_decay != 0:
        p = p + -weight_decay * lr * p
    if n_sma >= 5:
        return p + -step_size * lr * state["exp_avg"] / (np.sqrt(state["exp_avg_sq"]) + eps)
    return p + -step_size * lr * state["exp_avg"]


def run64(rule, kw, p0, gs, steps=STEPS):
    """`steps` steps over all tensors in float64 -> ([p], [state dict]).  gs[i][s] is None: tensor i has no gradient at step s (it
    is skipped and its own step count does not advance)."""
    ps, states, count = [np.asarray(p, np.float64) for p in p0], [dict() for _ in p0], [0] * len(p0)
    for s in range(steps):
        for i in range(len(ps)):
            if gs[i][s] is not None:
                count[i] += 1
                ps[i] = step64(rule, ps[i], gs[i][s], states[i], count[i], **kw)
    return ps, states


STATE_KEYS = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"), "adamw_ref": ("exp_avg", "exp_avg_sq")}
