"""RAdam, PlainRAdam and AdamW of the reference's utils/optim/radam.py.

RAdam with the reference's exact update rule (utils/optim/radam.py:6-98 of the reference): rectified Adam with an
SGD-style fallback while N_sma < 5 (the first 5 steps at beta2 = 0.999).  Device tensors are updated by the fused HIP
kernel kd_radam_step (one launch per tensor, no fp32 round-trip copies, no host sync); CPU tensors (the CIFAR plumbing
config) take an equivalent torch path.  The reference's 10-slot (step -> N_sma, step_size) cache is a pure function of
`step`, recomputed here (same values).

PlainRAdam (radam.py:101-176 of the reference) is RAdam without that cache: the same values, bit for bit, so it is RAdam here,
always through the multi-tensor launch.  AdamW (radam.py:179-250) is the reference's own class, NOT torch.optim.AdamW: a linear
learning-rate warm-up, a decay of weight_decay * scheduled_lr, eps added to sqrt(v) before the bias correction; device tensors
step through kd_optim_step_multi (KD_OPT_ADAMW_REF)."""
import math

import torch
from torch.optim.optimizer import Optimizer

from ... import ops


def _rect(step, beta1, beta2, degenerated_to_sgd=True):
    beta2_t = beta2 ** step
    n_max = 2 / (1 - beta2) - 1
    n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma >= 5:
        step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / \
            (1 - beta1 ** step)
    elif degenerated_to_sgd:
        step_size = 1.0 / (1 - beta1 ** step)
    else:
        step_size = -1
    return n_sma, step_size


class RAdam(Optimizer):
    _single_launch = True   # one tensor: kd_radam_step

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, degenerated_to_sgd=True):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        self.degenerated_to_sgd = degenerated_to_sgd
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        batch = []   # device tensors: one multi-tensor launch for all of them (kd_radam_step_multi)
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('RAdam does not support sparse gradients')
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                state['step'] += 1
                step = state['step']
                if p.is_cuda and p.dtype == torch.float32 and p.is_contiguous():
                    if not self.degenerated_to_sgd and _rect(step, beta1, beta2, False)[1] < 0:
                        # no parameter update this step, moments still advance (reference behaviour)
                        g = p.grad.float()
                        state['exp_avg_sq'].mul_(beta2).addcmul_(g, g, value=1 - beta2)
                        state['exp_avg'].mul_(beta1).add_(g, alpha=1 - beta1)
                        continue
                    g = p.grad if (p.grad.dtype == torch.float32 and p.grad.is_contiguous()) else p.grad.float().contiguous()
                    batch.append((p, g, state['exp_avg'], state['exp_avg_sq'], step, group['lr'], beta1, beta2,
                                  group['eps'], group['weight_decay']))
                    continue
                # torch path (CPU tensors)
                grad = p.grad.float()
                p32 = p.float()
                exp_avg, exp_avg_sq = state['exp_avg'], state['exp_avg_sq']
                exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
                n_sma, step_size = _rect(step, beta1, beta2, self.degenerated_to_sgd)
                if n_sma >= 5:
                    if group['weight_decay'] != 0:
                        p32.add_(p32, alpha=-group['weight_decay'] * group['lr'])
                    p32.addcdiv_(exp_avg, exp_avg_sq.sqrt().add_(group['eps']), value=-step_size * group['lr'])
                    p.copy_(p32)
                elif step_size > 0:
                    if group['weight_decay'] != 0:
                        p32.add_(p32, alpha=-group['weight_decay'] * group['lr'])
                    p32.add_(exp_avg, alpha=-step_size * group['lr'])
                    p.copy_(p32)
        if len(batch) == 1 and self._single_launch:
            ops.radam_step(*batch[0])
        elif batch:
            ops.radam_step_multi(batch)
        return loss


class PlainRAdam(RAdam):
    """The reference's PlainRAdam: RAdam's values (its (N_sma, step_size) cache is a pure function of `step`), the same state
    keys, the same no-update steps under degenerated_to_sgd=False; device tensors always step through kd_radam_step_multi."""
    _single_launch = False


class AdamW(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup=0):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, warmup=warmup))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        batch = []   # device tensors: one multi-tensor launch for all of them (kd_optim_step_multi)
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            lr, eps, wd, warmup = group['lr'], group['eps'], group['weight_decay'], group['warmup']
            hp = (float(lr), float(wd), float(eps), 0.0, 0.0, float(beta1), float(beta2), float(warmup))
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('Adam does not support sparse gradients, please consider SparseAdam instead')
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                state['step'] += 1
                step = state['step']
                if p.is_cuda and p.dtype == torch.float32 and p.is_contiguous():
                    g = p.grad if (p.grad.dtype == torch.float32 and p.grad.is_contiguous()) else p.grad.float().contiguous()
                    batch.append((p, g, (state['exp_avg'], state['exp_avg_sq']), step, 0, hp))
                    continue
                # torch path (CPU tensors)
                grad = p.grad.float()
                p32 = p.float()
                exp_avg, exp_avg_sq = state['exp_avg'], state['exp_avg_sq']
                exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
                denom = exp_avg_sq.sqrt().add_(eps)
                scheduled_lr = 1e-8 + step * lr / warmup if warmup > step else lr
                step_size = scheduled_lr * math.sqrt(1 - beta2 ** step) / (1 - beta1 ** step)
                if wd != 0:
                    p32.add_(p32, alpha=-wd * scheduled_lr)
                p32.addcdiv_(exp_avg, denom, value=-step_size)
                p.copy_(p32)
        ops.optim_step_multi("adamw_ref", batch)
        return loss
