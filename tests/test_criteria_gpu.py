"""The reference's JSDivergenceLoss, EnsembleKLDivergenceLoss, FocalLoss and TopkHintMSELoss on the GPU (kd_jsdiv, kd_jsdiv_up,
kd_ensemble_kldiv, kd_focal, kd_focal_grad, kd_focal_up, kd_topk_hint_mse): against the reference's own values and autograd
gradients (tests/golden/criteria.npz, tools/make_golden_criteria.py), against a float64 restatement at the full logit shape,
through LazyLogits and through LayerwiseTrainer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _criteria_ref as R  # noqa: E402
from _netutil import trainer_config  # noqa: E402
from _seeded import seeded_fill_, seeded_input  # noqa: E402
from test_criteria_host import focal_cases, focal_tag  # noqa: E402

FMTS = (torch.contiguous_format, torch.channels_last)


def _dev(a, fmt=torch.contiguous_format, dtype=torch.float32):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)
    return t.contiguous(memory_format=fmt) if t.dim() == 4 else t


def _bar(loss, grad, g, tag):
    loss = np.asarray(loss.detach().float().cpu().numpy())
    grad = grad.detach().float().cpu().numpy()
    np.testing.assert_allclose(loss, g[f"{tag}.loss"], rtol=1e-4, err_msg=tag)
    np.testing.assert_allclose(grad, g[f"{tag}.grad"], rtol=1e-3, atol=1e-7, err_msg=tag)


def _fused(crit, s, t):
    s = s.clone().requires_grad_(True)
    loss = crit(s, t)
    loss.backward()
    return loss, s.grad


@pytest.mark.parametrize("fmt", FMTS)
def test_jsd_ensemble_topk_match_the_reference(golden, fmt):
    from kdcc_amd import losses
    g = golden("criteria")
    for T in (1, 4):
        for tag in (f"jsd_T{T}", f"jsd2d_T{T}"):
            _bar(*_fused(losses.JSDivergenceLoss(T), _dev(g[f"{tag}.s"], fmt), _dev(g[f"{tag}.t"], fmt)), g, tag)
    _bar(*_fused(losses.EnsembleKLDivergenceLoss(), _dev(g["ekl.s"], fmt), _dev(g["ekl.t"], fmt)), g, "ekl")
    for Cc in (24, 64):
        for k in (0.5, 0.25):
            tag = f"topk_{Cc}_{k}"
            _bar(*_fused(losses.TopkHintMSELoss(topk=k), _dev(g[f"{tag}.s"], fmt), _dev(g[f"{tag}.t"], fmt)), g, tag)


@pytest.mark.parametrize("fmt", FMTS)
def test_focal_every_case_matches_the_reference(golden, fmt):
    from kdcc_amd import losses
    g = golden("criteria")
    x = _dev(g["focal.x"], fmt)
    for ign, gamma, red, an in focal_cases():
        tag = focal_tag(ign, gamma, red, an)
        tgt = _dev(g[f"focal.target_{'m100' if ign < 0 else ign}"]).long()
        alpha = torch.from_numpy(g["focal.alpha"]) if an == "alpha" else None
        crit = losses.FocalLoss(gamma, alpha=alpha, ignore_index=ign, reduction=red)
        s = x.clone().requires_grad_(True)
        loss = crit(s, tgt)
        if red == "none":
            assert loss.shape == (2, 2, 6, 8)
            loss.backward(_dev(g[f"{tag}.up"]))
        else:
            loss.backward()
        _bar(loss, s.grad, g, tag)


def test_bf16_operands_within_the_bf16_bars(golden):
    """bf16 operands against the float64 restatement evaluated on the bf16-rounded inputs, held to the existing bf16 loss bars
    (test_ops_gpu.py: test_losses_bf16_large_vs_oracle -- loss rtol 1e-4, gradient assert_close(..., "bf16"): max error 1.5e-2 of
    range and relative L2 5e-3; the gradient is stored in bf16)."""
    from test_ops_gpu import assert_close
    from kdcc_amd import losses
    g = golden("criteria")
    bf = torch.bfloat16

    def check(loss, grad, rl, rg, what):
        np.testing.assert_allclose(loss.item(), rl.item(), rtol=1e-4, err_msg=what)
        assert grad.dtype == bf
        assert_close(grad.float().cpu().numpy(), rg.cpu().numpy(), "bf16", what)

    for fmt in FMTS:
        for tag, crit, ref in (("jsd_T4", losses.JSDivergenceLoss(4), lambda s, t: R.jsd(s, t, 4)),
                               ("jsd2d_T1", losses.JSDivergenceLoss(1), lambda s, t: R.jsd(s, t, 1)),
                               ("ekl", losses.EnsembleKLDivergenceLoss(), R.ensemble_kl),
                               ("topk_64_0.25", losses.TopkHintMSELoss(topk=0.25), lambda s, t: R.topk_hint(s, t, 0.25))):
            s, t = _dev(g[f"{tag}.s"], fmt, bf), _dev(g[f"{tag}.t"], fmt, bf)
            check(*_fused(crit, s, t), *ref(s.float(), t.float()), f"{tag} {fmt}")
        tgt = _dev(g["focal.target_255"]).long()
        x = _dev(g["focal.x"], fmt, bf)
        alpha = torch.from_numpy(g["focal.alpha"])
        for gamma, red, a in ((2.0, "mean", alpha), (0.5, "sum", None), (0.0, "mean", alpha)):
            crit = losses.FocalLoss(gamma, alpha=a, ignore_index=255, reduction=red)
            check(*_fused(crit, x, tgt), *R.focal(x.float(), tgt, gamma, a, 255, red), f"focal {gamma} {red} {fmt}")


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def test_full_logit_shape_against_float64():
    """8 x 19 x 1024 x 2048 fp32 channels-last (the headline logits) and a 4096-channel 128 x 256 hint: loss and gradient within
    1e-4 of a float64 torch restatement computed on the GPU."""
    from kdcc_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(1)
    shape = (8, 19, 1024, 2048)
    cl = torch.channels_last
    s = (torch.randn(shape, device="cuda", generator=gen) * 3).contiguous(memory_format=cl)
    t = (torch.randn(shape, device="cuda", generator=gen) * 3).contiguous(memory_format=cl)
    loss, grad = ops.jsdiv(s, t, 4.0)
    rl, rg = R.jsd(s, t, 4.0)
    assert abs(loss.item() - rl.item()) <= 1e-4 * abs(rl.item()) and _rel(grad, rg) <= 1e-4
    del rl, rg
    pt = torch.softmax(t, 1).contiguous(memory_format=cl)
    loss, grad = ops.ensemble_kldiv(s, pt)
    rl, rg = R.ensemble_kl(s, pt)
    assert abs(loss.item() - rl.item()) <= 1e-4 * abs(rl.item()) and _rel(grad, rg) <= 1e-4
    del rl, rg, pt, t
    tgt = torch.randint(0, 19, (8, 1024, 2048), device="cuda", generator=gen)
    tgt[:, :64] = 255
    alpha = torch.rand(19, device="cuda", generator=gen) + 0.5
    loss, stats, _, _ = ops.focal(s, tgt, 2.0, alpha, 255, "mean")
    grad = ops.focal_grad(s, tgt, 2.0, alpha, 255, "mean", torch.ones((), device="cuda"), stats)
    rl, rg = R.focal(s, tgt, 2.0, alpha, 255, "mean")
    assert abs(loss.item() - rl.item()) <= 1e-4 * abs(rl.item()) and _rel(grad, rg) <= 1e-4
    del rl, rg, s, grad
    hs = torch.randn((2, 4096, 128, 256), device="cuda", generator=gen).contiguous(memory_format=cl)
    ht = torch.randn((2, 4096, 128, 256), device="cuda", generator=gen)
    ht = ht / ht.norm(dim=(-1, -2), keepdim=True)          # per-channel norms 1 + 0.01 * (a permutation): a pivot far above rounding
    perm = torch.stack([torch.randperm(4096, device="cuda", generator=gen) for _ in range(2)])
    ht = (ht * (1.0 + 0.01 * perm.float())[:, :, None, None]).contiguous(memory_format=cl)
    loss, grad, mask = ops.topk_hint_mse(hs, ht, 2048, want_mask=True)
    rm, _ = R.topk_mask(ht, 0.5)
    rl, rg = R.topk_hint(hs, ht, 0.5)
    assert torch.equal(mask.double(), rm)
    assert abs(loss.item() - rl.item()) <= 1e-4 * abs(rl.item()) and _rel(grad, rg) <= 1e-4


def test_two_calls_are_bitwise_equal():
    from kdcc_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(2)
    for fmt in FMTS:
        s = torch.randn((4, 19, 96, 160), device="cuda", generator=gen).contiguous(memory_format=fmt)
        t = torch.randn((4, 19, 96, 160), device="cuda", generator=gen).contiguous(memory_format=fmt)
        tgt = torch.randint(0, 19, (4, 96, 160), device="cuda", generator=gen)
        tgt[:, :5] = 255
        runs = []
        for _ in range(2):
            out = list(ops.jsdiv(s, t, 2.0)) + list(ops.ensemble_kldiv(s, torch.softmax(t, 1)))
            l, st, am, cm = ops.focal(s, tgt, 0.5, None, 255, "mean", want_maps=True)
            out += [l, st, am, cm, ops.focal_grad(s, tgt, 0.5, None, 255, "mean", torch.ones((), device="cuda"), st)]
            out += [x for x in ops.topk_hint_mse(s, t, 7, want_mask=True)]
            runs.append(out)
        for a, b in zip(*runs):
            assert torch.equal(a, b)


def test_low_resolution_forms_match_the_materialised_ones():
    """kd_jsdiv_up / kd_focal_up against kd_jsdiv / kd_focal on the up-sampled tensors, on test_lazy_logits_gpu.py's shapes."""
    from kdcc_amd import ops
    for (h, w, H, W, align) in [(12, 20, 24, 40, True), (23, 39, 46, 78, True), (16, 24, 31, 47, True), (12, 20, 24, 40, False),
                                (9, 300, 18, 600, True), (14, 22, 25, 40, False)]:
        gen = torch.Generator(device="cuda").manual_seed(h * 1000 + w)
        s_lo = torch.randn((2, h, w, 19), device="cuda", generator=gen) * 3
        t_lo = torch.randn((2, h, w, 19), device="cuda", generator=gen) * 3
        tgt = torch.randint(0, 19, (2, H, W), device="cuda", generator=gen)
        tgt[:, : max(1, H // 8)] = 255
        up = lambda lo: ops.upsample_bilinear_ac(lo, (H, W), out_dtype=torch.float32, align_corners=align).permute(0, 3, 1, 2)
        s_full, t_full = up(s_lo), up(t_lo)
        for T in (1.0, 4.0):
            ref, _ = ops.jsdiv(s_full, t_full, T, want_grad=False)
            np.testing.assert_allclose(ops.jsdiv_up(s_lo, t_lo, (H, W), T, align).item(), ref.item(), rtol=2e-5, atol=1e-7)
        alpha = torch.rand(19, device="cuda", generator=gen) + 0.5
        for gamma, red, a in ((2.0, "mean", None), (0.5, "sum", alpha), (0.0, "mean", alpha)):
            ref = ops.focal(s_full, tgt, gamma, a, 255, red)[0]
            got = ops.focal_up(s_lo, tgt, (H, W), gamma, a, 255, red, align)[0]
            np.testing.assert_allclose(got.item(), ref.item(), rtol=2e-5)


@pytest.mark.parametrize("align", [True, False])
def test_lazy_logits_back_propagated_through_deferred(align):
    """JSD and focal on pending LazyLogits take the half-resolution kernels; back-propagated, the deferred path gives the gradient
    the materialised criteria give."""
    from kdcc_amd import losses, ops
    from kdcc_amd.lazy import LazyLogits
    gen = torch.Generator(device="cuda").manual_seed(7)
    s_lo = torch.randn((2, 16, 24, 19), device="cuda", generator=gen) * 3
    t_lo = torch.randn((2, 16, 24, 19), device="cuda", generator=gen) * 3
    tgt = torch.randint(0, 19, (2, 32, 48), device="cuda", generator=gen)
    tgt[:, :4] = 255
    jsd, focal = losses.JSDivergenceLoss(2), losses.FocalLoss(2, ignore_index=255, reduction="mean")
    lz_s, lz_t = LazyLogits(s_lo, (32, 48), align), LazyLogits(t_lo, (32, 48), align)
    leaf = torch.zeros((), device="cuda", requires_grad=True)
    lz_s.anchor = leaf * 1.0
    loss = 0.7 * jsd(lz_s, lz_t) + 0.3 * focal(lz_s, tgt)
    assert lz_s.pending and lz_t.pending                          # the forward read only the half-resolution logits
    loss.backward()
    full = lambda lo: ops.upsample_bilinear_ac(lo, (32, 48), out_dtype=torch.float32, align_corners=align).permute(0, 3, 1, 2)
    s = full(s_lo).requires_grad_(True)
    loss_m = 0.7 * jsd(s, full(t_lo)) + 0.3 * focal(s, tgt)
    loss_m.backward()
    np.testing.assert_allclose(loss.item(), loss_m.item(), rtol=2e-5)
    np.testing.assert_allclose(lz_s.pending_grad.cpu().numpy(), s.grad.cpu().numpy(), rtol=1e-6, atol=1e-12)


def test_topk_ties_keep_the_lower_channel_and_k0_raises():
    from kdcc_amd import losses, ops
    gen = torch.Generator(device="cuda").manual_seed(9)
    base = torch.randn((2, 1, 6, 8), device="cuda", generator=gen)
    scale = torch.tensor([10.0, 9.0, 5.0, 8.0, 1.0, 5.0, 1.5, 2.0], device="cuda")   # channels 2 and 5: the same map
    for fmt in FMTS:
        t = (base * scale[None, :, None, None]).contiguous(memory_format=fmt)
        s = torch.randn((2, 8, 6, 8), device="cuda", generator=gen).contiguous(memory_format=fmt)
        _, _, mask = ops.topk_hint_mse(s, t, 4, want_mask=True)
        assert mask.tolist() == [[1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]] * 2
        loss, grad = _fused(losses.TopkHintMSELoss(topk=0.5), s, t)
        rl, rg = R.topk_hint(s, t, 0.5)
        np.testing.assert_allclose(loss.item(), rl.item(), rtol=1e-5)
        assert float(grad[:, 5].abs().max()) == 0.0 and float(grad[:, 2].abs().max()) > 0.0
        with pytest.raises(ValueError):
            losses.TopkHintMSELoss(topk=0.1)(s, t)           # int(0.1 * 8) == 0
        with pytest.raises(ValueError):
            ops.topk_hint_mse(s, t, 0)


def test_focal_gamma_below_one_at_certain_pixels():
    """gamma < 1 where p_y' == 1 in fp32: a == 0 and its gradient is the limit 0 (the reference's autograd gives NaN there)."""
    from kdcc_amd import losses
    gen = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn((2, 5, 4, 6), device="cuda", generator=gen)
    tgt = torch.randint(0, 5, (2, 4, 6), device="cuda", generator=gen)
    x[0, :, 1, :] = 0.0
    x[0, 3, 1, :] = 200.0          # p = 1 exactly ...
    tgt[0, 1, :] = 3               # ... for the labelled class
    for red in ("mean", "sum"):
        loss, grad = _fused(losses.FocalLoss(0.5, reduction=red), x, tgt)
        rl, rg = R.focal(x, tgt, 0.5, None, -100, red)
        assert torch.isfinite(grad).all()
        np.testing.assert_allclose(loss.item(), rl.item(), rtol=1e-4)
        np.testing.assert_allclose(grad.cpu().numpy(), rg.cpu().numpy(), rtol=1e-3, atol=1e-7)


def test_no_host_sync():
    from kdcc_amd import losses
    from kdcc_amd.lazy import LazyLogits
    gen = torch.Generator(device="cuda").manual_seed(6)
    s = torch.randn((2, 19, 32, 48), device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    t = torch.randn((2, 19, 32, 48), device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    pt = torch.softmax(t, 1)
    tgt = torch.randint(0, 19, (2, 32, 48), device="cuda", generator=gen)
    s_lo, t_lo = torch.randn((2, 16, 24, 19), device="cuda", generator=gen), torch.randn((2, 16, 24, 19), device="cuda", generator=gen)
    alpha = torch.rand(19, device="cuda", generator=gen)
    up = torch.randn((2, 2, 32, 48), device="cuda", generator=gen)
    crits = [losses.JSDivergenceLoss(4), losses.EnsembleKLDivergenceLoss(), losses.TopkHintMSELoss(),
             losses.FocalLoss(2, alpha=alpha, ignore_index=255, reduction="mean"), losses.FocalLoss(0.5, reduction="none")]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for c, tt in zip(crits, (t, pt, t, tgt, tgt)):
            x = s.clone().requires_grad_(True)
            loss = c(x, tt)
            loss.backward(up if loss.dim() else None)
        lz_s, lz_t = LazyLogits(s_lo, (32, 48)), LazyLogits(t_lo, (32, 48))
        losses.JSDivergenceLoss(1)(lz_s, lz_t)
        crits[3](lz_s, tgt)
        assert lz_s.pending
    finally:
        torch.cuda.set_sync_debug_mode(0)


def _trainer(tmp_path, backprop):
    from kdcc_amd import ConfigParser, losses, models
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer import LayerwiseTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    plan = ["mod4.block2.convs.conv2", "aspp.features.2.0"]
    cfg = trainer_config(plan, lr=1e-4, len_epoch=2, save_dir=str(tmp_path))
    cfg["kd_loss"] = {"type": "JSDivergenceLoss", "args": {"temperature": 2}}
    cfg["hint_loss"] = {"type": "TopkHintMSELoss", "args": {"topk": 0.5}}
    cfg["supervised_loss"] = {"type": "FocalLoss", "args": {"gamma": 2, "ignore_index": 255, "reduction": "mean"}}
    if backprop:
        cfg["trainer"]["backprop"] = backprop
    config = ConfigParser(cfg, run_id=f"crit_{backprop or 'a'}")
    teacher = config.init_obj("teacher", models)
    seeded_fill_(teacher, "teacher.")
    teacher.eval()
    model = DepthwiseStudent(teacher, config)
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    assert [type(c).__name__ for c in crit] == ["FocalLoss", "JSDivergenceLoss", "TopkHintMSELoss"]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    batches = []
    for i in range(2):
        tgt = torch.randint(0, 19, (1, 256, 512), generator=torch.Generator().manual_seed(30 + i))
        tgt[:, :16] = 255
        batches.append((seeded_input(f"crit.trainer.x{i}", (1, 3, 256, 512)), tgt))
    tr = LayerwiseTrainer(model, crit, [], opt, config, batches, None, sched, WeightScheduler(config["weight_scheduler"]))
    return tr, model, batches


@pytest.mark.parametrize("backprop", [None, "kd+hint"])
def test_layerwise_trainer_runs_the_new_criteria(tmp_path, backprop):
    tr, model, _ = _trainer(tmp_path, backprop)
    log = tr._train_epoch(1)
    for k in ("loss", "supervised_loss", "kd_loss", "hint_loss"):
        assert np.isfinite(log[k]) and log[k] > 0, (k, log[k])
    if backprop:
        assert abs(log["loss"] - log["kd_loss"] - log["hint_loss"]) < 1e-3 * abs(log["loss"])


class _LogitLayout(torch.autograd.Function):
    """Identity whose backward hands the gradient back in the channels-last layout of the engine's logits (the engine reads the
    logits' gradient in its own output layout; torch's softmax backward may return it NCHW-dense)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.contiguous(memory_format=torch.channels_last)


class _TorchJSD(torch.nn.Module):
    """The reference's JSDivergenceLoss.forward in stock torch autograd (targets detached, as the trainer's teacher logits are),
    evaluated in float64: with student and teacher this close, fp32 autograd through log(q) carries ~1e-5 of its own error."""

    def __init__(self, T):
        super().__init__()
        self.T = T

    def forward(self, inputs, targets):
        import torch.nn.functional as F
        T, t = self.T, targets.detach().double()
        inputs = _LogitLayout.apply(inputs).double()
        q = 0.5 * (F.softmax(t / T, dim=1) + F.softmax(inputs / T, dim=1))
        return T * T * 0.5 * (F.kl_div(torch.log(q), F.softmax(t / T, dim=1), reduction="sum") / t.shape[0] +
                              F.kl_div(torch.log(q), F.softmax(inputs / T, dim=1), reduction="sum") / t.shape[0]).float()


def test_mode_b_student_gradients_match_a_stock_torch_jsd(tmp_path):
    """Mode B, fp32: the student's parameter gradients of one step (kd + hint) with kd_jsdiv equal those with the KD criterion
    swapped for a stock-torch autograd JSD (rel-L2 <= 1e-5)."""
    tr, model, batches = _trainer(tmp_path, "kd+hint")
    tr.prepare_train_epoch(1)
    model.save_hidden = True
    x = batches[0][0].cuda()

    def grads(kd_crit):
        for p in model.student.parameters():
            p.grad = None
        out_st, out_tc = model(x)
        loss = kd_crit(out_st, out_tc) + tr._hint_loss()
        loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in model.student.named_parameters() if p.grad is not None}

    g_hip = grads(tr.criterions[1])
    g_ref = grads(_TorchJSD(2))
    assert g_hip and sorted(g_hip) == sorted(g_ref)
    bad = [(n, _rel(g_hip[n], g_ref[n])) for n in g_ref if _rel(g_hip[n], g_ref[n]) > 1e-5]
    assert not bad, bad[:10]
