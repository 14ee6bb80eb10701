"""Dropout on the GPU: kd_dropout_nhwc (csrc/dropout.hip) bit for bit against the numpy restatement of the rule in
tests/_dropoutref.py -- both kernels, padded and sliced views, the grid-stride loop, in place, the autograd function --, the mask's
statistics, and the networks that use it: the CIFAR Wide-ResNet (fp32 and bf16), the DenseNet and a ClassificationTrainer epoch.

The networks' reference is a float64 torch composition of the reference's expressions with the masks injected, one per block (layer)
in forward order; the masks are ops.dropout_nhwc of ones at the offsets nn_hip.dropout_state() says the forward drew.  Bars:
  * Wide-ResNet fp32: rel_l2 <= 1e-3 for the logits and for every parameter gradient, the tighter of the two bars tests/test_wrn_gpu.py
    has for them (1e-3 against the goldens, 1e-2 against float64 autograd at batch 4);
  * Wide-ResNet bf16: per quantity 2 x the rel_l2 of the bf16 emulation (tests/_wrn_bf16_ref.py with the dropout's store added) + 1e-6,
    the rule of tests/test_wrn_bf16_gpu.py;
  * DenseNet: rel_l2 <= 1e-3, tests/test_densenet_gpu.py's bar against float64 autograd."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _dropoutref as R  # noqa: E402
import _wrn_bf16_ref as E  # noqa: E402
from _netutil import trainer_config  # noqa: E402
from _seeded import seeded_fill_, seeded_input  # noqa: E402
from _wrnref import rel_l2  # noqa: E402

SEED = 123
BF = torch.bfloat16


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def ref_dropout(x, p, seed, offset):
    """Expected kd_dropout_nhwc output of a (..., C) host tensor (fp32 or bf16): tests/_dropoutref.py's rule."""
    Cc = x.shape[-1]
    flat = x.detach().cpu().contiguous().reshape(-1, Cc)
    kept = R.mask(seed, offset, flat.shape[0], Cc, p)
    if x.dtype == BF:
        out = R.apply_bf16(flat.view(torch.int16).numpy().view(np.uint16), kept, p)
        return torch.from_numpy(out.view(np.int16)).view(BF).reshape(x.shape)
    return torch.from_numpy(R.apply_f32(flat.numpy(), kept, p)).reshape(x.shape)


def same_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert torch.equal(bits(got), bits(want)), f"{what}: {(bits(got) != bits(want)).sum().item()} of {got.numel()} elements differ"


def last():
    from kdcc_amd import _lib
    return _lib.last_plumbing_kernel()


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("offset", [0, 1])
def test_vector_and_scalar_paths_dense(offset):
    from kdcc_amd import ops
    for shape, p, name in (((2, 8, 8, 16), 0.3, R.NAMES[1]), ((3, 5, 7, 10), 0.25, R.NAMES[0])):
        x = seeded_input(f"drop.{shape}", shape)
        xd = x.cuda()
        y = ops.dropout_nhwc(xd, p, SEED, offset)
        assert last() == name
        want = ref_dropout(x, p, SEED, offset)
        same_bits(y, want, f"{shape} out of place")
        assert torch.equal(xd.cpu(), x), "the input changed"
        assert ops.dropout_nhwc(xd, p, SEED, offset, out=xd) is xd and last() == name
        same_bits(xd, want, f"{shape} in place")
        kept = (want != 0).float().mean().item()
        assert abs(kept - (1 - p)) < 0.1


@pytest.mark.parametrize("offset", [0, 1])
def test_bf16_padded_buffer_keeps_its_zero_tail(offset):
    """C = 160 in an ld = 192 buffer (the Wide-ResNet's bf16 activations): the vector kernel, pad channels neither read nor written."""
    from kdcc_amd import nn_hip, ops
    x = seeded_input("drop.bf16.x", (2, 8, 8, 160)).to(BF)
    xv = nn_hip.new_padded((2, 8, 8, 160), "cuda", BF)
    yv = nn_hip.new_padded((2, 8, 8, 160), "cuda", BF)
    assert xv.stride(2) == yv.stride(2) == 192
    xv.copy_(x.cuda())
    whole = lambda v: v.as_strided((2, 8, 8, 192), v.stride())
    whole(xv)[..., 160:] = float("nan")          # (a pad channel that was read would not matter; one that was copied would show)
    y = ops.dropout_nhwc(xv, 0.3, SEED, offset, out=yv)
    assert last() == R.NAMES[3]
    want = ref_dropout(x, 0.3, SEED, offset)
    same_bits(y, want, "bf16 padded")
    assert int(bits(whole(yv)[..., 160:]).abs().max()) == 0, "a pad channel of the output was written"
    whole(xv)[..., 160:] = 0
    ops.dropout_nhwc(xv, 0.3, SEED, offset, out=xv)
    same_bits(xv, want, "bf16 padded, in place")
    assert int(bits(whole(xv)[..., 160:]).abs().max()) == 0
    # the mask does not depend on the dtype: the fp32 call keeps the same elements
    y32 = ops.dropout_nhwc(x.float().cuda(), 0.3, SEED, offset)
    assert torch.equal(y32.cpu() != 0, want.float() != 0)


@pytest.mark.parametrize("offset", [0, 1])
def test_slice_of_a_wider_buffer_and_the_scalar_kernel_on_the_same_mask(offset):
    """C = 32 from a dense temporary into channels [64:96) of an ld = 96 buffer (a dense block's slice): the vector kernel, the other
    channels untouched.  The same call through a view at channel offset 1, and with ld = 97: each closes one gate, the scalar kernel
    runs, the result is the same bits."""
    from kdcc_amd import ops
    x = seeded_input("drop.slice.x", (2, 8, 8, 32))
    xd = x.cuda()
    want = ref_dropout(x, 0.3, SEED, offset)
    fill = seeded_input("drop.slice.buf", (2, 8, 8, 98))
    for ld, c0, name in ((96, 64, R.NAMES[1]), (96, 1, R.NAMES[0]), (97, 0, R.NAMES[0]), (97, 64, R.NAMES[0]), (98, 2, R.NAMES[0])):
        buf = fill[..., :ld].contiguous().cuda()
        keep = buf.cpu().clone()
        y = ops.dropout_nhwc(xd, 0.3, SEED, offset, out=buf[..., c0:c0 + 32])
        assert last() == name, (ld, c0)
        same_bits(y, want, f"ld {ld} channel offset {c0}")
        after = buf.cpu()
        assert torch.equal(bits(after[..., :c0]), bits(keep[..., :c0])) and torch.equal(bits(after[..., c0 + 32:]), bits(keep[..., c0 + 32:])), \
            f"ld {ld} channel offset {c0}: a channel outside the slice changed"
        # ... and read back through the strided view (the backward's pass over a slice of the gradient)
        z = ops.dropout_nhwc(buf[..., c0:c0 + 32], 0.3, SEED, offset)
        assert last() == name
        same_bits(z, ref_dropout(want, 0.3, SEED, offset), f"ld {ld} channel offset {c0}, strided input")


def test_more_items_than_one_stride_of_the_capped_grid():
    """M * C / 4 = 2048 * 256 + 37 lanes' worth in both kernels: the second trip of the grid-stride loop, and a partial last block."""
    from kdcc_amd import ops
    M = R.CAP * R.TPB + 37
    x = seeded_input("drop.stride.x", (1, 1, M, 4))
    want = ref_dropout(x, 0.3, SEED, 0)
    y = ops.dropout_nhwc(x.cuda(), 0.3, SEED, 0)
    assert last() == R.NAMES[1] and R.predict(R.F32, M, 4, 0, 4, 0, 4)[2:] == (M, R.CAP)
    same_bits(y, want, "vector kernel")
    wide = torch.zeros((1, 1, M, 5), device="cuda")
    wide[..., :4] = x.cuda()
    z = ops.dropout_nhwc(wide[..., :4], 0.3, SEED, 0)
    assert last() == R.NAMES[0]
    same_bits(z, want, "scalar kernel")
    M3 = (4 * R.CAP * R.TPB + 1) // 3                                     # 3 M3 = 4 (CAP TPB) + 1 elements: a last block of 1
    assert 3 * M3 == 4 * R.CAP * R.TPB + 1 and R.predict(R.BF16, M3, 3, 0, 3, 0, 3)[2:] == (R.CAP * R.TPB + 1, R.CAP)
    x3 = seeded_input("drop.stride.x3", (1, 1, M3, 3)).to(BF)
    z3 = ops.dropout_nhwc(x3.cuda(), 0.3, SEED, 1)
    assert last() == R.NAMES[2]
    same_bits(z3, ref_dropout(x3, 0.3, SEED, 1), "scalar bf16 kernel")


def test_the_autograd_function_regenerates_the_mask():
    from kdcc_amd import nn_hip
    nn_hip.seed_dropout(SEED, 5)
    x = seeded_input("drop.fn.x", (2, 16, 8, 8)).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gy = seeded_input("drop.fn.gy", (2, 16, 8, 8)).cuda().contiguous(memory_format=torch.channels_last)
    y = nn_hip.dropout(x, 0.3, True)
    assert nn_hip.dropout_state() == (SEED, 6), "one draw per forward"
    assert getattr(y, nn_hip._PADDED, 0) == 32 and y.permute(0, 2, 3, 1).stride(2) == 32, "the result lives in a padded, tagged buffer"
    assert int(bits(y.permute(0, 2, 3, 1).as_strided((2, 8, 8, 32), y.permute(0, 2, 3, 1).stride())[..., 16:]).abs().max()) == 0
    assert not y.grad_fn.saved_tensors, "no mask and no activation is stored"
    y.backward(gy)
    assert nn_hip.dropout_state() == (SEED, 6), "the backward draws nothing"
    same_bits(y.permute(0, 2, 3, 1), ref_dropout(x.detach().permute(0, 2, 3, 1).cpu(), 0.3, SEED, 5), "forward")
    same_bits(x.grad.permute(0, 2, 3, 1), ref_dropout(gy.permute(0, 2, 3, 1).cpu(), 0.3, SEED, 5), "dx = gy * mask * scale")
    assert nn_hip.dropout(x, 0.3, False) is x and nn_hip.dropout(x, 0.0, True) is x and nn_hip.dropout_state() == (SEED, 6)


@pytest.mark.parametrize("p", [0.2, 0.3, 0.85])
def test_mask_statistics(p):
    """M = 65536, C = 16 at seed 123.  (The numpy rule alone stays under 2 sigma on all of these: worst 1.63.)"""
    from kdcc_amd import ops
    M, Cc = 65536, 16
    ones = torch.ones((64, 32, 32, Cc), device="cuda")
    m0 = ops.dropout_nhwc(ones, p, SEED, 0) != 0
    m1 = ops.dropout_nhwc(ones, p, SEED, 1) != 0
    assert np.array_equal(m0.cpu().numpy().reshape(M, Cc), R.mask(SEED, 0, M, Cc, p)), "the kernel's mask is not the rule's"
    n = M * Cc
    center = 1.0 - R.params(p)[0] / 2.0 ** 32
    sigma = lambda q, k: (q * (1 - q) / k) ** 0.5
    for name, m in (("offset 0", m0), ("offset 1", m1)):
        share = m.double().mean().item()
        print(f"DROPSTAT p={p} {name}: kept {share:.6f} expected {center:.6f} ({abs(share - center) / sigma(p, n):.2f} sigma)")
        assert abs(share - center) <= 4 * sigma(p, n), name
        per_c = m.reshape(M, Cc).double().mean(0).cpu()
        worst = float((per_c - center).abs().max())
        print(f"DROPSTAT p={p} {name}: worst channel {worst / sigma(p, M):.2f} sigma")
        assert worst <= 4.5 * sigma(p, M), name
    agree, a = (m0 == m1).double().mean().item(), p * p + (1 - p) * (1 - p)
    print(f"DROPSTAT p={p}: offsets 0 and 1 agree on {agree:.6f}, expected {a:.6f} ({abs(agree - a) / sigma(a, n):.2f} sigma)")
    assert abs(agree - a) <= 4 * sigma(a, n)


# ------------------------------------------------------------------------------------------------------------- Wide-ResNet
WRN = dict(depth=10, widen_factor=2, num_classes=10)


class DropNet(E.Net):
    """tests/_wrn_bf16_ref.py's network with the reference's F.dropout between relu2(bn2(conv1)) and conv2 as a multiplication by the
    injected mask * scale, one per block in forward order; the dropout stores its output (and its input gradient) once: an R."""

    def __init__(self, depth, masks, emulate):
        super().__init__(depth, emulate)
        self.masks = masks

    def forward(self, sd, x, training=False):
        self.block = 0
        return super().forward(sd, x, training)

    def conv(self, sd, name, a, stride=1, padding=1, res=None):
        if name.endswith(".conv2"):
            a = self.R(a * self.masks[self.block])
            self.block += 1
        return super().conv(sd, name, a, stride, padding, res)


def drawn_masks(state0, state1, shapes, p):
    """mask * scale (float64, NCHW, on the host) of every draw between two readings of nn_hip.dropout_state(): ops.dropout_nhwc of ones."""
    from kdcc_amd import ops
    assert state0[0] == state1[0] and state1[1] - state0[1] == len(shapes), (state0, state1, len(shapes))
    return [ops.dropout_nhwc(torch.ones(s, device="cuda"), p, state0[0], state0[1] + i).permute(0, 3, 1, 2).double().cpu() for i, s in enumerate(shapes)]


def count_launches(monkeypatch):
    from kdcc_amd import ops
    calls = []
    orig = ops.dropout_nhwc
    monkeypatch.setattr(ops, "dropout_nhwc", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


def wrn_run(net, x, w):
    out = net(x)
    (out * w).sum().backward()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_wrn_train_logits_and_every_gradient(dtype):
    from kdcc_amd import nn_hip
    from kdcc_amd.models.cifar_models import wrn
    m = seeded_fill_(wrn(dropRate=0.3, **WRN), "wrn.drop.")
    x, w = seeded_input("wrn.drop.x", (4, 3, 32, 32)), seeded_input("wrn.drop.w", (4, 10))
    net = copy.deepcopy(m).cuda().train()
    nn_hip.seed_dropout(SEED)
    s0 = nn_hip.dropout_state()
    out = wrn_run(net, x.cuda().to(dtype=dtype, memory_format=torch.channels_last), w.cuda())
    s1 = nn_hip.dropout_state()
    masks = drawn_masks(s0, s1, [(4, 32, 32, 32), (4, 16, 16, 64), (4, 8, 8, 128)], 0.3)
    assert all(0.6 < float((k != 0).double().mean()) < 0.8 for k in masks)

    def reference(emulate):
        sd = E.double_sd(m)
        o = DropNet(WRN["depth"], masks, emulate).forward(sd, x.double(), training=True)
        (o * w.double()).sum().backward()
        return o.detach(), {k: v.grad for k, v in sd.items() if v.requires_grad}
    exact_out, exact_grad = reference(False)
    assert out.dtype == torch.float32
    if dtype == torch.float32:
        bars = {"logits": 1e-3, **{n: 1e-3 for n in exact_grad}}
    else:
        em_out, em_grad = reference(True)
        bars = {"logits": 2 * rel_l2(em_out, exact_out) + 1e-6, **{n: 2 * rel_l2(em_grad[n], exact_grad[n]) + 1e-6 for n in exact_grad}}
    missed = []
    for name, got, ref in [("logits", out, exact_out)] + [(n, p.grad, exact_grad[n]) for n, p in net.named_parameters()]:
        err = rel_l2(got.detach().double().cpu(), ref)
        print(f"DROPWRN {dtype} {name}: rel_l2 {err:.3e} bar {bars[name]:.3e}")
        if not err <= bars[name]:
            missed.append(f"{name}: rel_l2 {err:.3e} > {bars[name]:.3e}")
    assert not missed, missed
    # without the masks the reference is far away: the comparison sees the dropout
    sd = E.double_sd(m)
    plain = E.Net(WRN["depth"], False).forward(sd, x.double(), training=True).detach()
    assert rel_l2(out.detach().double().cpu(), plain) > 0.05


def test_wrn_eval_and_rate_zero_launch_and_draw_nothing(monkeypatch):
    from kdcc_amd import nn_hip
    from kdcc_amd.models.cifar_models import wrn
    m = seeded_fill_(wrn(dropRate=0.3, **WRN), "wrn.drop.")
    m0 = wrn(dropRate=0.0, **WRN)
    m0.load_state_dict(m.state_dict())
    x = seeded_input("wrn.drop.x", (4, 3, 32, 32)).cuda()
    nn_hip.seed_dropout(SEED, 3)
    calls = count_launches(monkeypatch)
    a, b = copy.deepcopy(m).cuda().eval(), copy.deepcopy(m0).cuda().eval()
    with torch.no_grad():
        assert torch.equal(a(x), b(x)), "eval mode, fused chain"
    assert torch.equal(a(x), b(x)), "eval mode, module path"
    t0 = copy.deepcopy(m0).cuda().train()
    wrn_run(t0, x, seeded_input("wrn.drop.w", (4, 10)).cuda())
    assert not calls and nn_hip.dropout_state() == (SEED, 3), "eval mode and dropRate = 0 launch nothing and draw nothing"
    t1 = copy.deepcopy(m).cuda().train()
    wrn_run(t1, x, seeded_input("wrn.drop.w", (4, 10)).cuda())
    assert len(calls) == 6 and nn_hip.dropout_state() == (SEED, 6), "three blocks: three forward passes, three backward passes, three draws"


def test_wrn_same_seed_same_bits_another_seed_not():
    from kdcc_amd import nn_hip
    from kdcc_amd.models.cifar_models import wrn
    m = seeded_fill_(wrn(dropRate=0.3, **WRN), "wrn.drop.")
    x, w = seeded_input("wrn.drop.x", (4, 3, 32, 32)).cuda(), seeded_input("wrn.drop.w", (4, 10)).cuda()

    def run(seed, through_torch):
        net = copy.deepcopy(m).cuda().train()
        if through_torch:
            torch.manual_seed(seed)
        else:
            nn_hip.seed_dropout(seed)
        out = wrn_run(net, x, w)
        return out.detach(), [p.grad for p in net.parameters()]
    keep = torch.initial_seed()
    try:
        o1, g1 = run(7, False)
        o2, g2 = run(7, False)
        assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
        o3, g3 = run(8, False)
        assert not torch.equal(o1, o3) and not torch.equal(g1[0], g3[0])
        o4, g4 = run(7, True)            # torch.manual_seed(7) alone: the stream restarts at (7, 0)
        assert nn_hip.dropout_state() == (7, 3) and torch.equal(o1, o4) and all(torch.equal(a, b) for a, b in zip(g1, g4))
    finally:
        torch.manual_seed(keep)


# ------------------------------------------------------------------------------------------------------------- DenseNet
DN = dict(growth_rate=8, bn_size=2, block_config=(2, 1, 1, 1), num_init_features=16, drop_rate=0.2)
DN_LAYERS = [(1, 1, 16), (1, 2, 16), (2, 1, 8), (3, 1, 4), (4, 1, 2)]          # (block, layer, map size)


def densenet_drop_forward(sd, x, masks, taps):
    """tests/_densenetref.densenet_forward in train mode with each layer's new features multiplied by its mask * scale."""
    bn = lambda p, t: F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], True, 0.1, 1e-5)
    out = F.conv2d(x, sd["features.conv0.weight"], padding=1)
    out = F.max_pool2d(F.relu(bn("features.norm0", out)), 3, 2, 1)
    masks = iter(masks)
    for k, n in enumerate(DN["block_config"], 1):
        for j in range(1, n + 1):
            p = f"features.denseblock{k}.denselayer{j}"
            h = F.conv2d(F.relu(bn(p + ".norm1", out)), sd[p + ".conv1.weight"])
            new = F.conv2d(F.relu(bn(p + ".norm2", h)), sd[p + ".conv2.weight"], padding=1)
            taps[p + ".conv2"] = new
            new = new * next(masks)
            taps[p + ".dropped"] = new
            out = torch.cat([out, new], 1)
        if k != len(DN["block_config"]):
            p = f"features.transition{k}"
            out = F.avg_pool2d(F.conv2d(F.relu(bn(p + ".norm", out)), sd[p + ".conv.weight"]), 2, 2)
    out = F.relu(bn("features.norm5", out))
    return F.linear(F.adaptive_avg_pool2d(out, 1).flatten(1), sd["classifier.weight"], sd["classifier.bias"])


def test_densenet_train_logits_gradients_and_what_the_hooks_see():
    from kdcc_amd import nn_hip
    from kdcc_amd.models.cifar_models import DenseNet
    m = seeded_fill_(DenseNet(**DN), "dn.drop.")
    x, w = seeded_input("dn.drop.x", (2, 3, 32, 32)), seeded_input("dn.drop.w", (2, 10))
    net = copy.deepcopy(m).cuda().train()
    seen = {}
    for name in ("features.denseblock1.denselayer1.conv2", "features.denseblock1"):
        net.get_submodule(name).register_forward_hook(lambda mod, i, o, name=name: seen.__setitem__(name, o))
    nn_hip.seed_dropout(SEED)
    s0 = nn_hip.dropout_state()
    out = net(x.cuda())
    (out * w.cuda()).sum().backward()
    s1 = nn_hip.dropout_state()
    masks = drawn_masks(s0, s1, [(2, hw, hw, 8) for _, _, hw in DN_LAYERS], 0.2)
    sd = {k: v.clone().double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in m.state_dict().items()}
    taps = {}
    ref = densenet_drop_forward(sd, x.double(), masks, taps)
    (ref * w.double()).sum().backward()
    missed = []
    pre, blk = seen["features.denseblock1.denselayer1.conv2"].detach(), seen["features.denseblock1"].detach()
    checks = [("logits", out, ref), ("hook on denselayer1.conv2 (before the dropout)", pre, taps["features.denseblock1.denselayer1.conv2"]),
              ("block output slice [16:24]", blk[:, 16:24], taps["features.denseblock1.denselayer1.dropped"]),
              ("block output slice [24:32]", blk[:, 24:32], taps["features.denseblock1.denselayer2.dropped"])]
    checks += [("grad " + n, p.grad, sd[n].grad) for n, p in net.named_parameters()]
    for name, got, want in checks:
        err = rel_l2(got.detach().double().cpu(), want.detach())
        print(f"DROPDN {name}: rel_l2 {err:.3e}")
        if not err <= 1e-3:
            missed.append(f"{name}: rel_l2 {err:.3e} > 1e-3")
    assert not missed, missed
    # exactly: the slice is the dropout of what the hook saw, and the hook did not see the dropped features
    want = ref_dropout(pre.permute(0, 2, 3, 1).cpu(), 0.2, s0[0], s0[1])
    same_bits(blk[:, 16:24].permute(0, 2, 3, 1), want, "the slice is the dropout of the hooked features")
    assert float((pre == 0).double().mean()) < 0.01 < 0.1 < float((blk[:, 16:24] == 0).double().mean()) < 0.3


def test_densenet_layer_with_a_cheap_conv_block_runs():
    from kdcc_amd import nn_hip
    from kdcc_amd.models.cifar_models import DenseNet
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    net = seeded_fill_(DenseNet(**DN), "dn.drop.")
    layer = net.features.denseblock1.denselayer1
    layer.conv2 = seeded_fill_(DepthwiseSeparableBlock(16, 8, 3, 1, 1, 16, None), "dn.drop.cheap.")
    net = net.cuda().train()
    seen = {}
    layer.conv2.register_forward_hook(lambda mod, i, o: seen.__setitem__("pre", o))
    net.features.denseblock1.register_forward_hook(lambda mod, i, o: seen.__setitem__("blk", o))
    nn_hip.seed_dropout(SEED)
    out = net(seeded_input("dn.drop.x", (2, 3, 32, 32)).cuda())
    (out * seeded_input("dn.drop.w", (2, 10)).cuda()).sum().backward()
    assert nn_hip.dropout_state() == (SEED, 5) and torch.isfinite(out).all()
    want = ref_dropout(seen["pre"].detach().permute(0, 2, 3, 1).cpu(), 0.2, SEED, 0)
    same_bits(seen["blk"].detach()[:, 16:24].permute(0, 2, 3, 1), want, "the slice is the dropout of the cheap block's output")
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    g = layer.conv2.pointwise_conv.weight.grad
    assert float(g.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------- ClassificationTrainer
SMALL = dict(depth=10, widen_factor=4, num_classes=100)
PLAN = {"hint": ["block3.layer.0"], "unfreeze": ["block3.layer.0"], "pruning_plan": ["block3.layer.0.conv2"]}


def _config(save_dir, drop):
    cfgd = trainer_config([], lr=0.1, len_epoch=1, save_dir=save_dir)         # (the trainer runs len_epoch + 1 iterations: two batches)
    cfgd.update(name="dropout_wrn", teacher={"type": "wrn", "args": dict(SMALL, dropRate=drop)}, optimizer={"type": "SGD", "args": {"lr": 0.1}},
                kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
                hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}}, metrics=["accuracy", "top_k_acc"],
                lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}})
    cfgd["trainer"]["name"] = "ClassificationTrainer"
    cfgd["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3}, **{k: [{"name": n, "epoch": 1} for n in v] for k, v in PLAN.items()}}
    return cfgd


def _epoch(save_dir, run_id, seed):
    from kdcc_amd import ConfigParser, losses, nn_hip
    from kdcc_amd.models import cifar_models, metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer import ClassificationTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    config = ConfigParser(_config(save_dir, 0.3), run_id=run_id)
    teacher = seeded_fill_(config.init_obj("teacher", cifar_models), "wrn.").cuda().eval()
    assert teacher.block1.layer[0].droprate == 0.3
    model = DepthwiseStudent(teacher, config)
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"wrn.student.{b['name']}.")
    model.replace = replace_and_seed
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(metric, k) for k in config["metrics"]]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    batches = [(seeded_input(f"wrn.tr.x{i}", (8, 3, 32, 32)), torch.randint(0, 100, (8,), generator=torch.Generator().manual_seed(300 + i)))
               for i in range(2)]
    tr = ClassificationTrainer(model, crit, metrics, opt, config, batches, None, sched, WeightScheduler(config["weight_scheduler"]))
    nn_hip.seed_dropout(seed)
    log = tr._train_epoch(1)
    drawn = nn_hip.dropout_state()[1]
    return log, {n: p.detach().clone() for n, p in model.student.named_parameters() if p.requires_grad}, drawn, teacher


def test_classification_trainer_epoch_with_dropout(tmp_path):
    from kdcc_amd.models import cifar_models
    log1, par1, drawn, teacher = _epoch(str(tmp_path / "a"), "a", 11)
    log2, par2, drawn2, _ = _epoch(str(tmp_path / "b"), "b", 11)
    assert drawn == drawn2 == 2 * 3, "the train-mode student draws once per block and batch; the eval-mode teacher draws nothing"
    for k in ("loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss"):
        assert np.isfinite(log1[k]) and log1[k] == log2[k], (k, log1[k], log2[k])
    assert par1 and all(torch.equal(par1[n], par2[n]) for n in par1)
    log3, _, _, _ = _epoch(str(tmp_path / "c"), "c", 12)
    assert log3["kd_loss"] != log1["kd_loss"], "another seed, other masks"
    plain = cifar_models.wrn(dropRate=0.0, **SMALL)
    plain.load_state_dict(teacher.state_dict())
    x = seeded_input("wrn.tr.x0", (8, 3, 32, 32)).cuda()
    with torch.no_grad():
        assert torch.equal(teacher(x), plain.cuda().eval()(x)), "the eval-mode teacher is the dropRate = 0 teacher"
