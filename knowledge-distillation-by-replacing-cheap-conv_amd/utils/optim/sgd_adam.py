"""torch.optim.SGD and torch.optim.Adam with the step on this package's own kernel (kd_optim_step_multi, csrc/optim.hip).

The classes ARE torch's -- constructor, validation, defaults, param_groups, add_param_group, state_dict / load_state_dict and
__setstate__ are inherited -- and only `step` is overridden.  The state keys and types are torch's (`momentum_buffer`; `step` as
the fp32 CPU scalar tensor torch keeps, read without a device sync; `exp_avg`, `exp_avg_sq`, `max_exp_avg_sq`), so a checkpoint
written by either class loads into the other and a run may change paths midway.

The kernel path is taken when every parameter that has a gradient is an fp32 contiguous tensor on the current device with a
dense gradient and no group asks for capturable / differentiable / fused=True (or holds a hyper-parameter as a Tensor).  Anything
else -- CPU tensors (host plumbing runs, n_gpu: 0), bf16, non-contiguous or empty parameters, sparse gradients -- is torch's own step
for the whole optimizer, bit for bit.  A closure runs first, as in torch, and the path is chosen from the gradients it leaves."""
import torch

from ... import ops


def _torch_step(cls):
    """torch's own step of `cls` without the step hooks Optimizer wraps round it (they already run round ours)."""
    fn = cls.step
    return fn.__wrapped__ if getattr(fn, "hooked", False) else fn


def _number(*xs):
    return all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in xs)


def _dev_f32(t, device):
    return t.dtype == torch.float32 and t.device == device and t.layout == torch.strided and t.is_contiguous()


def _kernel_params(opt, state_keys):
    """[(group, [params with a gradient])] if the kernel can take this step, else None.  Decides only; mutates nothing."""
    if not torch.cuda.is_available():
        return None
    device, out = None, []
    for group in opt.param_groups:
        if group.get("capturable") or group.get("differentiable") or group.get("fused") or group.get("decoupled_weight_decay"):
            return None
        betas = group.get("betas", (0.0, 0.0))
        if not _number(group["lr"], group["weight_decay"], group.get("momentum", 0.0), group.get("dampening", 0.0),
                       group.get("eps", 0.0), *betas):
            return None
        ps = []
        for p in group["params"]:
            if p.grad is None:
                continue
            if device is None:
                if not p.is_cuda or p.device.index != torch.cuda.current_device():
                    return None
                device = p.device
            if not _dev_f32(p, device) or p.grad.layout != torch.strided or p.grad.device != device or p.numel() == 0:
                return None
            st = opt.state.get(p)
            if st:
                for k in state_keys:
                    if k in st and st[k] is not None and not _dev_f32(st[k], device):
                        return None
                if "step" in st and not (torch.is_tensor(st["step"]) and st["step"].device.type == "cpu"):
                    return None
            ps.append(p)
        out.append((group, ps))
    return out


def _grad(p):
    g = p.grad
    return g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()


class SGD(torch.optim.SGD):
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:   # first, as in torch: the gradients the step sees are the ones the closure leaves
            with torch.enable_grad():
                loss = closure()
        plan = _kernel_params(self, ("momentum_buffer",))
        if plan is None:
            _torch_step(torch.optim.SGD)(self, None)
            return loss
        items = []
        for group, ps in plan:
            momentum = group["momentum"]
            base = (ops.OPT_NESTEROV if group["nesterov"] else 0) | (ops.OPT_MAXIMIZE if group["maximize"] else 0)
            hp = (float(group["lr"]), float(group["weight_decay"]), 0.0, float(momentum), float(group["dampening"]), 0.0, 0.0, 0.0)
            for p in ps:
                if momentum == 0:
                    items.append((p, _grad(p), (), 0, base, hp))
                    continue
                state = self.state[p]
                buf = state.get("momentum_buffer")
                if buf is None:   # torch: buf = clone(g) on the first step; here the kernel writes g into a fresh buffer
                    buf = state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                    items.append((p, _grad(p), (buf,), 0, base | ops.OPT_FIRST, hp))
                else:
                    items.append((p, _grad(p), (buf,), 0, base, hp))
        ops.optim_step_multi("sgd", items)
        return loss


class Adam(torch.optim.Adam):
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:   # first, as in torch: the gradients the step sees are the ones the closure leaves
            with torch.enable_grad():
                loss = closure()
        plan = _kernel_params(self, ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
        if plan is None:
            _torch_step(torch.optim.Adam)(self, None)
            return loss
        items = []
        for group, ps in plan:
            beta1, beta2 = group["betas"]
            amsgrad = group["amsgrad"]
            flags = (ops.OPT_AMSGRAD if amsgrad else 0) | (ops.OPT_MAXIMIZE if group["maximize"] else 0)
            hp = (float(group["lr"]), float(group["weight_decay"]), float(group["eps"]), 0.0, 0.0, float(beta1), float(beta2), 0.0)
            for p in ps:
                state = self.state[p]
                if len(state) == 0:   # torch's lazy state initialisation (adam.py, _init_group)
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if amsgrad:
                        state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1
                states = (state["exp_avg"], state["exp_avg_sq"]) + ((state["max_exp_avg_sq"],) if amsgrad else ())
                items.append((p, _grad(p), states, int(state["step"].item()), flags, hp))
        ops.optim_step_multi("adam", items)
        return loss
