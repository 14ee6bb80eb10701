"""Stock-torch restatement of the CIFAR pre-activation ResNet forward, written from the architecture (every conv reads
relu(bn(.)) of its input; the stride sits on conv1 of a basic block and on the 3x3 conv2 of a bottleneck; where a block has a
1x1 `downsample.0` conv it reads the RAW block input with the block's stride; the net ends in bn, relu, mean over the 8x8 map,
fc) over a plain state dict, for the host-plumbing, gradient and full-size tests."""
import torch.nn.functional as F


def _bn(sd, p, x, training, momentum=0.1, eps=1e-5):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], training,
                        momentum, eps)


def preresnet_forward(sd, x, training=False):
    """Logits of a PreResNet with the parameters / buffers in `sd` (train mode updates its running statistics).  Depth and block
    type are read off the keys."""
    bottleneck = "layer1.0.conv3.weight" in sd
    n = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layer1."))
    out = F.conv2d(x, sd["conv1.weight"], padding=1)
    for g in (1, 2, 3):
        for i in range(n):
            p = f"layer{g}.{i}"
            stride = 2 if (g > 1 and i == 0) else 1
            h = F.relu(_bn(sd, p + ".bn1", out, training))
            if bottleneck:
                h = F.relu(_bn(sd, p + ".bn2", F.conv2d(h, sd[p + ".conv1.weight"]), training))
                h = F.relu(_bn(sd, p + ".bn3", F.conv2d(h, sd[p + ".conv2.weight"], stride=stride, padding=1), training))
                h = F.conv2d(h, sd[p + ".conv3.weight"])
            else:
                h = F.relu(_bn(sd, p + ".bn2", F.conv2d(h, sd[p + ".conv1.weight"], stride=stride, padding=1), training))
                h = F.conv2d(h, sd[p + ".conv2.weight"], padding=1)
            sc = F.conv2d(out, sd[p + ".downsample.0.weight"], stride=stride) if (p + ".downsample.0.weight") in sd else out
            out = sc + h
    out = F.relu(_bn(sd, "bn", out, training))
    out = F.avg_pool2d(out, 8).flatten(1)
    return F.linear(out, sd["fc.weight"], sd["fc.bias"])
