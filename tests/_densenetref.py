"""Stock-torch restatement of the CIFAR DenseNet-BC forward, written from the architecture (3x3 stem + BN + ReLU + 3x3/2 max
pool; dense layers BN-ReLU-1x1-BN-ReLU-3x3 whose output is concatenated to their input; transitions BN-ReLU-1x1-2x2 average
pool; final BN, ReLU, global average pool, linear) over a plain state dict in fp32 or fp64, train or eval mode, for the
host-plumbing, concat-free and full-width tests."""
import torch
import torch.nn.functional as F

from _wrnref import project, rel_l2  # noqa: F401  (the DenseNet goldens store the same seeded projections)

DENSENET121 = (6, 12, 24, 16)
SMALL = dict(growth_rate=32, block_config=(2, 2, 2, 2), num_init_features=64, num_classes=10)


def _bn(sd, p, x, training, momentum=0.1, eps=1e-5):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], training,
                        momentum, eps)


def densenet_forward(sd, x, block_config=DENSENET121, training=False, taps=None):
    """Logits of DenseNet(block_config=...) with the parameters / buffers in `sd` (dtype of `sd`; train mode updates its running
    statistics).  taps: a dict that receives every 'features.denseblockK.denselayerJ' output (the concatenation) and
    'features.denseblockK.denselayerJ.conv2' output."""
    out = F.conv2d(x, sd["features.conv0.weight"], padding=1)
    out = F.max_pool2d(F.relu(_bn(sd, "features.norm0", out, training)), 3, 2, 1)
    for k, n in enumerate(block_config, 1):
        for j in range(1, n + 1):
            p = f"features.denseblock{k}.denselayer{j}"
            h = F.conv2d(F.relu(_bn(sd, p + ".norm1", out, training)), sd[p + ".conv1.weight"])
            new = F.conv2d(F.relu(_bn(sd, p + ".norm2", h, training)), sd[p + ".conv2.weight"], padding=1)
            out = torch.cat([out, new], 1)
            if taps is not None:
                taps[p + ".conv2"] = new
                taps[p] = out
        if k != len(block_config):
            p = f"features.transition{k}"
            out = F.avg_pool2d(F.conv2d(F.relu(_bn(sd, p + ".norm", out, training)), sd[p + ".conv.weight"]), 2, 2)
    out = F.relu(_bn(sd, "features.norm5", out, training))
    return F.linear(F.adaptive_avg_pool2d(out, 1).flatten(1), sd["classifier.weight"], sd["classifier.bias"])


def bound(g, name, floor=1e-3):
    """The test bound of a stored tensor: max(floor, 3 x the reference's own fp32-vs-fp64 rel-L2 error of it)."""
    return max(floor, 3.0 * float(g["tol:" + name]))
