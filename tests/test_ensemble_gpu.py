"""kd_kldiv_multi / kd_softmax_mean and EnsembleTrainer on the GPU: against the reference's own values and autograd gradients
(tests/golden/ensemble.npz, tools/make_golden_ensemble.py), against the float64 restatement in tests/_ensemble_ref.py, against the
sibling kernels they fuse, and the trainer's epoch, launch count, fallback and checkpoint round trip."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ensemble_ref as R  # noqa: E402
from _ensemble_util import (MEMBER_PLANS, build_trainer, crit_case, ensemble_config, member_checkpoint, seeded_teacher,  # noqa: E402
                            trainer_batches, wrn_config)
from _seeded import seeded_fill_, seeded_input  # noqa: E402
from _wrnref import project, rel_l2  # noqa: E402

CL = torch.channels_last


def _bar(vals, grad, g, key):
    """test_criteria_gpu._bar: scalars rtol 1e-4, gradient rtol 1e-3 / atol 1e-7."""
    kd, sup, total = (float(v) for v in vals)
    print(key, "kd", kd, g[f"{key}.kd"], "sup", sup, g[f"{key}.sup"], "total", total, g[f"{key}.loss"],
          "grad max err", float(np.abs(grad.float().cpu().numpy() - g[f"{key}.grad"]).max()))
    np.testing.assert_allclose(kd, g[f"{key}.kd"], rtol=1e-4, err_msg=key)
    np.testing.assert_allclose(sup, g[f"{key}.sup"], rtol=1e-4, err_msg=key)
    np.testing.assert_allclose(total, g[f"{key}.loss"], rtol=1e-4, err_msg=key)
    np.testing.assert_allclose(grad.float().cpu().numpy(), g[f"{key}.grad"], rtol=1e-3, atol=1e-7, err_msg=key)


def _fmt(t, fmt):
    return t.contiguous(memory_format=fmt) if t.dim() == 4 else t


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("case", ["2d", "nchw", "channels_last"])
def test_kldiv_multi_matches_the_reference(golden, case, T):
    from kdcc_amd import ops
    g = golden("ensemble")
    tag = "crit2d" if case == "2d" else "crit4d"
    fmt = CL if case == "channels_last" else torch.contiguous_format
    s, ts, labels, w = crit_case(g, tag, "cuda")
    kd, sup, total, grad = ops.kldiv_multi(_fmt(s, fmt), [_fmt(t, fmt) for t in ts], w, T, labels, 255)
    assert grad.stride() == _fmt(s, fmt).stride()
    _bar((kd, sup, total), grad, g, f"{tag}_T{T}")
    # scales: total and gradient are linear in them
    kd2, sup2, total2, grad2 = ops.kldiv_multi(_fmt(s, fmt), [_fmt(t, fmt) for t in ts], w, T, labels, 255, kd_scale=0.25, sup_scale=0.5)
    assert torch.equal(kd2, kd) and torch.equal(sup2, sup)
    np.testing.assert_allclose(float(total2), 0.25 * float(kd) + 0.5 * float(sup), rtol=1e-6)
    r = R.kldiv_multi(s, ts, w, T, labels, 255, 0.25, 0.5)
    assert rel_l2(grad2, r["grad"]) <= 1e-4
    # forward only
    kd3, sup3, total3, none = ops.kldiv_multi(_fmt(s, fmt), [_fmt(t, fmt) for t in ts], w, T, labels, 255, want_grad=False)
    assert none is None and torch.equal(kd3, kd) and torch.equal(sup3, sup) and torch.equal(total3, total)


def test_kldiv_multi_many_pixels_few_classes_takes_the_staged_path():
    """Dense channels-last with C < 22 and >= 16384 pixels (the 256-pixel LDS tiles, a ragged last tile) and its NCHW twin (the
    one-pixel-per-thread kernel) against the float64 restatement, T = 2, mixed fp32 / bf16 targets."""
    from kdcc_amd import ops
    shape = (3, 19, 75, 77)
    s = seeded_input("ens.big.s", shape, 2.0).cuda()
    ts = [seeded_input(f"ens.big.t{k}", shape, 2.0).cuda() for k in range(3)]
    ts[1] = ts[1].bfloat16()
    labels = torch.randint(0, 19, (3, 75, 77), generator=torch.Generator().manual_seed(5)).cuda()
    labels[:, :7] = 255
    w = [1.0, 0.5, 3.0]
    r = R.kldiv_multi(s, [t.float() for t in ts], w, 2.0, labels, 255)
    for fmt in (CL, torch.contiguous_format):
        kd, sup, total, grad = ops.kldiv_multi(_fmt(s, fmt), [_fmt(t, fmt) for t in ts], w, 2.0, labels, 255)
        for got, key in ((kd, "kd"), (sup, "sup"), (total, "total")):
            np.testing.assert_allclose(float(got), r[key].item(), rtol=1e-4, err_msg=f"{key} {fmt}")
        np.testing.assert_allclose(grad.cpu().numpy(), r["grad"].cpu().numpy(), rtol=1e-3, atol=1e-7)


def test_kldiv_multi_bf16_operands_within_the_bf16_bars(golden):
    from test_ops_gpu import assert_close
    from kdcc_amd import ops
    g = golden("ensemble")
    bf = torch.bfloat16
    for tag, fmt in (("crit2d", torch.contiguous_format), ("crit4d", torch.contiguous_format), ("crit4d", CL)):
        s, ts, labels, w = crit_case(g, tag, "cuda")
        s, ts = _fmt(s.to(bf), fmt), [_fmt(t.to(bf), fmt) for t in ts]
        for T in (1, 5):
            kd, sup, total, grad = ops.kldiv_multi(s, ts, w, T, labels, 255)
            r = R.kldiv_multi(s.float(), [t.float() for t in ts], w, T, labels, 255)
            for got, key in ((kd, "kd"), (sup, "sup"), (total, "total")):
                np.testing.assert_allclose(float(got), r[key].item(), rtol=1e-4, err_msg=f"{tag} {key}")
            assert grad.dtype == bf
            assert_close(grad.float().cpu().numpy(), r["grad"].cpu().numpy(), "bf16", f"{tag} T{T} {fmt}")


def test_kldiv_multi_one_target_equals_the_sibling_kernels(golden):
    from kdcc_amd import ops
    g = golden("ensemble")
    for tag, fmt in (("crit2d", torch.contiguous_format), ("crit4d", torch.contiguous_format), ("crit4d", CL)):
        s, ts, labels, _ = crit_case(g, tag, "cuda")
        s, t = _fmt(s, fmt), _fmt(ts[0], fmt)
        for T in (1.0, 5.0):
            kd, sup, total, grad = ops.kldiv_multi(s, [t], [0.7], T, labels, 255)
            kl, gkl = ops.kldiv(s, t, T)
            ce, gce = ops.ce2d(s, labels, 255), ops.ce2d_grad(s, labels, 255)
            np.testing.assert_allclose(float(kd), float(kl), rtol=1e-4)
            np.testing.assert_allclose(float(sup), float(ce), rtol=1e-4)
            np.testing.assert_allclose(float(total), float(kl) + float(ce), rtol=1e-4)
            np.testing.assert_allclose(grad.cpu().numpy(), (gkl + gce).cpu().numpy(), rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("n_t", [1, 6, 16])
@pytest.mark.parametrize("shape", [(128, 100), (128, 10), (5, 300), (2, 7, 9, 11)], ids=["128x100", "128x10", "5x300", "2x7x9x11"])
def test_kldiv_multi_target_counts_and_two_runs_bitwise(n_t, shape):
    from kdcc_amd import ops
    s = seeded_input("ens.n.s", shape, 2.0).cuda()
    ts = [seeded_input(f"ens.n.t{k}", shape, 2.0).cuda() for k in range(n_t)]
    w = [1.0 + 0.25 * k for k in range(n_t)]
    C = shape[1]
    labels = torch.randint(0, C, (shape[0],) + shape[2:], generator=torch.Generator().manual_seed(n_t)).cuda()
    labels.view(-1)[::5] = 255
    a = ops.kldiv_multi(s, ts, w, 3.0, labels, 255)
    b = ops.kldiv_multi(s, ts, w, 3.0, labels, 255)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    r = R.kldiv_multi(s, ts, w, 3.0, labels, 255)
    for got, key in zip(a[:3], ("kd", "sup", "total")):
        np.testing.assert_allclose(float(got), r[key].item(), rtol=1e-4, err_msg=key)
    np.testing.assert_allclose(a[3].cpu().numpy(), r["grad"].cpu().numpy(), rtol=1e-3, atol=1e-7)


def test_kldiv_multi_refuses_0_and_17_targets_and_survives_all_ignored(golden):
    from kdcc_amd import ops
    from kdcc_amd._lib import KdccError
    g = golden("ensemble")
    s, ts, labels, w = crit_case(g, "crit4d", "cuda")
    with pytest.raises(KdccError, match="1 to 16"):
        ops.kldiv_multi(s, [], [], 1.0)
    with pytest.raises(KdccError, match="1 to 16"):
        ops.kldiv_multi(s, [ts[0]] * 17, [1.0] * 17, 1.0)
    with pytest.raises(KdccError, match="1 to 16"):
        ops.softmax_mean([ts[0]] * 17, [1.0] * 17, 1.0)
    with pytest.raises(KdccError):
        ops.kldiv_multi(s, ts, [0.0, 0.0, 0.0], 1.0)
    ok = ops.kldiv_multi(s, ts, w, 1.0)                          # the device is fine afterwards
    for fmt in (torch.contiguous_format, CL):
        kd, sup, total, grad = ops.kldiv_multi(_fmt(s, fmt), [_fmt(t, fmt) for t in ts], w, 1.0, torch.full_like(labels, 255), 255)
        assert float(sup) == 0.0 and torch.isfinite(grad).all() and torch.equal(kd, ok[0])
        np.testing.assert_allclose(grad.cpu().numpy(), ok[3].cpu().numpy(), rtol=1e-6, atol=1e-9)
    s2, ts2, labels2, w2 = crit_case(g, "crit2d", "cuda")
    kd, sup, total, grad = ops.kldiv_multi(s2, ts2, w2, 5.0, torch.full_like(labels2, 255), 255)
    assert float(sup) == 0.0 and torch.isfinite(grad).all() and float(total) == float(kd)


def test_softmax_mean_rows_sum_to_one_and_feeds_the_ensemble_kl(golden):
    from kdcc_amd import losses, ops
    g = golden("ensemble")
    for tag, fmt in (("crit2d", torch.contiguous_format), ("crit4d", torch.contiguous_format), ("crit4d", CL)):
        s, ts, _, w = crit_case(g, tag, "cuda")
        ts = [_fmt(t, fmt) for t in ts]
        for T in (1.0, 5.0):
            p = ops.softmax_mean(ts, w, T)
            assert p.dtype == torch.float32 and p.stride() == ts[0].stride()
            ref = R.softmax_mean(ts, w, T)
            np.testing.assert_allclose(p.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-9)
            assert float((p.double().sum(1) - 1).abs().max()) <= 1e-6
        p = ops.softmax_mean(ts, w, 1.0)
        sg = _fmt(s, fmt).clone().requires_grad_(True)
        loss = losses.EnsembleKLDivergenceLoss()(sg, p)
        loss.backward()
        # KL(mean || softmax(s)) at T = 1: the restatement's per-target sum minus the targets' entropy terms, so state it directly
        pm = R.softmax_mean(ts, w, 1.0)
        lps = torch.log_softmax(s.double(), 1)
        NP = s.numel() // s.shape[1]
        np.testing.assert_allclose(float(loss.detach()), float((torch.xlogy(pm, pm) - pm * lps).sum() / NP), rtol=1e-4)
        assert rel_l2(sg.grad, (lps.exp() - pm) / NP) <= 1e-4
        # ... whose gradient is the multi-target gradient (linear in the targets)
        assert rel_l2(sg.grad, R.kldiv_multi(s, ts, w, 1.0)["grad"]) <= 1e-4
    big = [seeded_input(f"ens.sm.{k}", (3, 19, 75, 77), 2.0).cuda().bfloat16().contiguous(memory_format=CL) for k in range(2)]
    p = ops.softmax_mean(big, [1.0, 2.0], 2.0)
    np.testing.assert_allclose(p.cpu().numpy(), R.softmax_mean([b.float() for b in big], [1.0, 2.0], 2.0).cpu().numpy(), rtol=1e-4, atol=1e-9)


# ------------------------------------------------------------------------------------------------ the trainer
@pytest.fixture
def trainer(tmp_path):
    paths = [member_checkpoint(i, plan, str(tmp_path)) for i, plan in enumerate(MEMBER_PLANS)]
    return build_trainer(ensemble_config(str(tmp_path), paths))


def test_ensemble_predict_and_epoch_match_the_reference(golden, trainer):
    g = golden("ensemble")
    tr = trainer
    assert len(tr.models) == int(g["n_members"])
    x0 = tr.valid_data_loader[0][0].cuda()
    pred = tr.ensemble_predict(x0)
    np.testing.assert_allclose(pred.cpu().numpy(), g["predict"], rtol=1e-4, atol=1e-6)
    assert float((pred.double().sum(1) - 1).abs().max()) <= 1e-6
    log = tr._train_epoch(1)
    assert sorted(log) == list(g["train_keys"])
    for k in g["train_keys"]:
        print(k, log[k], float(g[f"train:{k}"]))
    for k in g["train_keys"]:
        np.testing.assert_allclose(log[k], float(g[f"train:{k}"]), rtol=2e-3, atol=1e-6, err_msg=k)
    for n, p in tr.model.student.named_parameters():
        assert p.requires_grad
        assert rel_l2(project(p.data, n), g[f"param:{n}"]) <= 1e-3, n
    test_log = tr._test_epoch(1)
    assert sorted(test_log) == list(g["test_keys"])
    for k in ("accuracy", "top_k_acc"):
        assert test_log[k] == pytest.approx(float(g[f"test:{k}"]), abs=1e-9), k
    # validation interval reached: the single student's and the ensemble's metrics join the log under their prefixes
    tr.do_validation_interval = 1
    log2 = tr._train_epoch(2)
    assert {"val_accuracy", "val_top_k_acc", "ensemble_accuracy", "ensemble_top_k_acc"} <= set(log2)


def test_one_criterion_launch_per_step_and_the_fallback_loop(trainer, monkeypatch):
    from kdcc_amd import losses, ops
    tr = trainer
    calls = {}

    def counted(name):
        fn = getattr(ops, name)

        def wrapper(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapper)
    for name in ("kldiv", "ce2d", "ce2d_grad", "kldiv_multi", "jsdiv"):
        counted(name)
    prof = []
    monkeypatch.setattr(ops, "PROFILER", prof)
    tr._train_epoch(1)                                        # len_epoch + 1 = 3 steps
    torch.cuda.synchronize()
    assert calls == {"kldiv_multi": 3}, calls
    assert [p[5] for p in prof if p[0] == "loss"] == ["kd_kldiv_multi"] * 3
    monkeypatch.setattr(ops, "PROFILER", None)

    # any other criterion pair: the reference's loop over the criterion modules, here JSD
    calls.clear()
    tr.criterions[1] = losses.JSDivergenceLoss(temperature=4).cuda()
    tr.prepare_models(2)
    data, target = (t.cuda() for t in trainer_batches()[0])
    output_st, output_tc = tr.model(data)
    with torch.no_grad():
        outputs = [m(data) for m in tr.models]
    loss, log_loss, log_sup, log_kd = tr._criterion(output_st, output_tc, outputs, target)
    assert calls.get("jsdiv") == 3 and calls.get("ce2d") == 1 and "kldiv_multi" not in calls
    import _criteria_ref as CR
    want_kd = sum(CR.jsd(output_st, t, 4)[0] for t in outputs + [output_tc]) / 3
    want_sup = R.kldiv_multi(output_st, [output_tc], [1.0], 1.0, target, 255)["sup"]
    np.testing.assert_allclose(float(log_kd), float(want_kd), rtol=1e-4)
    np.testing.assert_allclose(float(log_sup), float(want_sup), rtol=1e-4)
    np.testing.assert_allclose(float(loss), float(want_kd + want_sup), rtol=1e-4)
    g_logits, = torch.autograd.grad(loss, output_st)
    want_g = sum(CR.jsd(output_st, t, 4)[1] for t in outputs + [output_tc]) / 3 + \
        R.kldiv_multi(output_st, [output_tc], [1.0], 1.0, target, 255, kd_scale=0.0)["grad"]
    assert rel_l2(g_logits, want_g) <= 1e-4


def test_fused_criterion_with_gradient_accumulation(trainer):
    """accumulation_steps = 2: loss and gradient halve, the logged values do not."""
    tr = trainer
    tr.prepare_models(1)
    data, target = (t.cuda() for t in trainer_batches()[0])
    output_st, output_tc = tr.model(data)
    with torch.no_grad():
        outputs = [m(data) for m in tr.models]
    tr.accumulation_steps = 2
    loss, log_loss, log_sup, log_kd = tr._criterion(output_st, output_tc, outputs, target)
    g_logits, = torch.autograd.grad(loss, output_st)
    r = R.kldiv_multi(output_st, outputs + [output_tc], [1.0, 1.0, 1.0], 5.0, target, 255, 0.5, 0.5)
    np.testing.assert_allclose(float(loss), r["total"].item(), rtol=1e-4)
    np.testing.assert_allclose(float(log_loss), 2 * r["total"].item(), rtol=1e-4)
    np.testing.assert_allclose(float(log_kd), r["kd"].item(), rtol=1e-4)
    np.testing.assert_allclose(float(log_sup), r["sup"].item(), rtol=1e-4)
    assert rel_l2(g_logits, r["grad"]) <= 1e-4


def test_real_checkpoint_round_trip(tmp_path):
    """ClassificationTrainer trains the reduced WRN for one epoch and saves through _save_checkpoint (config: a pickled ConfigParser);
    EnsembleTrainer resumes from that file."""
    from kdcc_amd import ConfigParser, losses
    from kdcc_amd.models import metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.models.students.transform_blocks import DepthwiseSeparableBlock
    from kdcc_amd.trainer import ClassificationTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    config = ConfigParser(wrn_config("c5", str(tmp_path / "cls")), run_id="cls")
    model = DepthwiseStudent(seeded_teacher().cuda(), config)
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    ct = ClassificationTrainer(model, crit, metrics, opt, config, trainer_batches(), None, sched, WeightScheduler(config["weight_scheduler"]))
    ct._train_epoch(1)
    ct._save_checkpoint(1)
    path = ct.checkpoint_dir / "checkpoint-epoch1.pth"
    assert path.exists()
    trained = {k: v.detach().clone() for k, v in model.student.state_dict().items()}
    tr = build_trainer(ensemble_config(str(tmp_path / "ens"), [str(path)]), run_id="rt")
    assert len(tr.models) == 1
    member = tr.models[0]
    assert isinstance(member.block2.layer[0].conv2, DepthwiseSeparableBlock)
    got = member.state_dict()
    assert set(got) == set(trained) and all(torch.equal(got[k], trained[k]) for k in trained)
    assert not torch.equal(trained["block2.layer.0.conv1.weight"], tr.model.teacher.state_dict()["block2.layer.0.conv1.weight"])
    log = tr._train_epoch(1)
    assert np.isfinite([log["loss"], log["kd_loss"], log["supervised_loss"]]).all()
