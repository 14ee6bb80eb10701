"""Stock-torch restatements (float64, any device) of the four criteria of losses/JSDiv.py, EnsembleKLDiv.py, FocalLoss.py and
WeightedHintMSELoss.py:19-44 of the reference, written from their formulas (include/kdcc.h, losses section): value and gradient
w.r.t. the first operand."""
import math

import torch
import torch.nn.functional as F


def _d(x):
    return x.detach().to(torch.float64)


def jsd(s, t, T):
    s, t = _d(s), _d(t)
    N = s.shape[0]
    lps, lpt = F.log_softmax(s / T, 1), F.log_softmax(t / T, 1)
    ps, pt = lps.exp(), lpt.exp()
    lq = math.log(0.5) + torch.logaddexp(lps, lpt)
    loss = T * T / (2 * N) * (torch.xlogy(ps, ps) + torch.xlogy(pt, pt) - (ps + pt) * lq).sum()
    a = lps - lq
    grad = T / (2 * N) * ps * (a - (ps * a).sum(1, keepdim=True))
    return loss, grad


def ensemble_kl(s, t):
    s, t = _d(s), _d(t)
    NP = s.numel() // s.shape[1]
    lps = F.log_softmax(s, 1)
    loss = (torch.xlogy(t, t) - t * lps).sum() / NP
    grad = (lps.exp() * t.sum(1, keepdim=True) - t) / NP
    return loss, grad


def focal(x, target, gamma, alpha=None, ignore_index=-100, reduction="none", upstream=None):
    """-> (loss, grad); for 'none' the loss is the (N,N,*sp) product and grad is for the upstream (N,N,*sp) gradient."""
    x = _d(x)
    N, C = x.shape[:2]
    xs = x.reshape(N, C, -1)
    tg = target.reshape(N, -1)
    valid = (tg != ignore_index) & (tg >= 0) & (tg < C)
    yv = torch.where(valid, tg, torch.zeros_like(tg))
    lp = F.log_softmax(xs, 1)
    p = lp.exp()
    py = p.gather(1, yv[:, None])[:, 0]
    a = (1 - py) ** gamma
    w = torch.ones(C, dtype=torch.float64, device=x.device) if alpha is None else _d(alpha).to(x.device)
    wy = torch.where(valid, w[yv], torch.zeros_like(py))
    ce = -wy * lp.gather(1, yv[:, None])[:, 0]
    NP = a.numel()
    onehot_g = F.one_hot(yv, C).permute(0, 2, 1).to(torch.float64)
    om = 1 - py
    if gamma == 0:
        coef = torch.zeros_like(py)
    else:
        coef = torch.where(om > 0, -gamma * om.clamp_min(1e-300) ** (gamma - 1) * py, torch.zeros_like(py))
    da = coef[:, None] * (onehot_g - p)                          # d a / d x
    dce = wy[:, None] * (p - onehot_g)                           # d ce / d x (0 at ignored pixels)
    if reduction == "mean":
        ce_mean = ce.sum() / wy.sum()
        loss = a.mean() * ce_mean
        grad = ce_mean / NP * da + a.mean() / wy.sum() * dce
    elif reduction == "sum":
        loss = a.sum() * ce.sum()
        grad = ce.sum() * da + a.sum() * dce
    else:
        sp = tuple(x.shape[2:])
        loss = (a[:, None, :] * ce[None, :, :]).reshape(N, N, *sp)
        G = _d(upstream).reshape(N, N, -1)
        ua = (G * ce[None]).sum(1)
        uc = (G * a[:, None]).sum(0)
        grad = ua[:, None] * da + uc[:, None] * dce
        return loss, grad.reshape(x.shape)
    if upstream is not None:
        grad = grad * _d(upstream)
    return loss, grad.reshape(x.shape)


def topk_mask(t, topk):
    """(N,C) mask of each sample's int(topk * C) channels of largest L2 norm; equal norms keep the lower channel."""
    t = _d(t)
    N, C = t.shape[:2]
    k = int(topk * C)
    norm = t.reshape(N, C, -1).pow(2).sum(-1)
    # stable descending sort: among equal norms the lower index comes first
    idx = torch.sort(norm, dim=1, descending=True, stable=True).indices[:, :k]
    mask = torch.zeros(N, C, dtype=torch.float64, device=t.device)
    mask.scatter_(1, idx, 1.0)
    return mask, k


def topk_hint(s, t, topk):
    s, t = _d(s), _d(t)
    N, C = s.shape[:2]
    P = s[0, 0].numel()
    mask, k = topk_mask(t, topk)
    d = s - t
    loss = (mask * d.pow(2).reshape(N, C, -1).mean(-1)).sum() / (N * k)
    grad = 2 * mask[:, :, None, None] * d / (P * N * k)
    return loss, grad
