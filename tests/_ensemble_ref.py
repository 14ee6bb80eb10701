"""Stock-torch restatements (float64, any device) of kd_kldiv_multi and kd_softmax_mean, written from their formulas
(include/kdcc.h, losses section): the ensemble step's criterion of trainer/ensemble_trainer.py:80-85 and ensemble_predict (:145-164)
of the reference."""
import torch
import torch.nn.functional as F


def _d(x):
    return x.detach().to(torch.float64)


def kldiv_multi(s, targets, weights, T, labels=None, ignore_index=255, kd_scale=1.0, sup_scale=1.0):
    """-> dict(kd_each [one KLDivergenceLoss(T) value per target], kd, sup, total, grad = d total / d s)."""
    s = _d(s)
    N, C = s.shape[:2]
    NP = s.numel() // C
    W = float(sum(weights))
    lps = F.log_softmax(s / T, 1)
    each, q = [], torch.zeros_like(s)
    for t, w in zip(targets, weights):
        lpt = F.log_softmax(_d(t) / T, 1)
        pt = lpt.exp()
        each.append(T * T / NP * (torch.xlogy(pt, pt) - pt * lps).sum())
        q = q + (w / W) * pt
    kd = sum(w / W * e for w, e in zip(weights, each))
    grad = kd_scale * T / NP * (lps.exp() - q)
    sup = torch.zeros((), dtype=torch.float64, device=s.device)
    if labels is not None:
        valid = (labels != ignore_index) & (labels >= 0) & (labels < C)
        nvalid = int(valid.sum())
        if nvalid:
            lp1 = F.log_softmax(s, 1)
            y = torch.where(valid, labels, torch.zeros_like(labels)).unsqueeze(1)
            sup = -(lp1.gather(1, y).squeeze(1) * valid).sum() / nvalid
            onehot = torch.zeros_like(s).scatter_(1, y, 1.0)
            grad = grad + sup_scale / nvalid * (lp1.exp() - onehot) * valid.unsqueeze(1)
    return {"kd_each": each, "kd": kd, "sup": sup, "total": kd_scale * kd + sup_scale * sup, "grad": grad}


def softmax_mean(logits, weights, T):
    W = float(sum(weights))
    return sum((w / W) * torch.softmax(_d(x) / T, 1) for x, w in zip(logits, weights))
