"""Stock-torch restatement of the CIFAR Wide-ResNet forward, written from the architecture (pre-activation basic blocks;
where a block changes width its 1x1 shortcut and its first conv both read relu(bn1(x)), elsewhere the shortcut is x) over a
plain state dict, for the host-plumbing and full-width tests.  Plus the seeded random projections the WRN goldens store in
place of large tensors."""
import torch
import torch.nn.functional as F

from _seeded import seeded_input


def _bn(sd, p, x, training, momentum=0.1, eps=1e-5):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], training,
                        momentum, eps)


def wrn_forward(sd, x, depth=28, training=False):
    """Logits of WideResNet(depth, ...) with the parameters / buffers in `sd` (train mode updates its running statistics)."""
    n = (depth - 4) // 6
    out = F.conv2d(x, sd["conv1.weight"], padding=1)
    for g in (1, 2, 3):
        for i in range(n):
            p = f"block{g}.layer.{i}"
            stride = 2 if (g > 1 and i == 0) else 1
            a = F.relu(_bn(sd, p + ".bn1", out, training))
            h = F.relu(_bn(sd, p + ".bn2", F.conv2d(a, sd[p + ".conv1.weight"], stride=stride, padding=1), training))
            h = F.conv2d(h, sd[p + ".conv2.weight"], padding=1)
            sc = F.conv2d(a, sd[p + ".convShortcut.weight"], stride=stride) if (p + ".convShortcut.weight") in sd else out
            out = sc + h
    out = F.relu(_bn(sd, "bn1", out, training))
    out = F.adaptive_avg_pool2d(out, 1).flatten(1)
    return F.linear(out, sd["fc.weight"], sd["fc.bias"])


def project(t, key, k=64):
    """k seeded random projections of t (fp64): what the goldens store for tensors too large to keep whole."""
    f = t.detach().double().cpu().reshape(-1)
    return seeded_input("proj." + key, (k, f.numel())).double() @ f


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
