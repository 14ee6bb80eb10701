"""kd_cifar_batch and the device-resident CIFAR loaders on the GPU.  The kernel is a gather, so every comparison is torch.equal: against
the host path of the same loader (the vectorised torch composition of the same table) and against the per-image PIL oracle of
tests/_cifar_loader_ref.py; labels and every byte of the zero tail of the "padded" layout included.  Then the path the batches take:
a reduced Wide-ResNet reads a "padded" batch without a padding copy, a ClassificationTrainer epoch fed by the loader logs the losses
of the same epoch fed by a list of the same batches, and a batch made on a side stream is whole once that stream is."""
import pytest
import torch

import _cifar_loader_ref as R
from _netutil import trainer_config
from _seeded import seeded_fill_

gpu = pytest.mark.gpu
BF = torch.bfloat16
LAYOUTS = ("nchw", "nhwc", "padded")
DTYPES = {"fp32": torch.float32, "bf16": BF}
SMALL = dict(depth=10, widen_factor=4, num_classes=100)
LOSSES = ("loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """name -> (root, images, labels): CIFAR-100 training files of 37, 300 and 64 images."""
    out = {}
    for n in (37, 300, 64):
        root = str(tmp_path_factory.mktemp(f"c100_{n}"))
        tr, trl, _, _ = R.write_cifar100(root, n, 1, seed=n)
        out[n] = (root, tr, trl)
    return out


def loader(root, batch, device, **kw):
    from kdcc_amd import data_loader
    kw.setdefault("seed", 0)
    return data_loader.Cifar100Dataloader(root, batch, device=device, **kw)


def whole(batch):
    """The batch's storage as the kernel wrote it: the (B,32,32,ld) buffer of an NHWC / padded batch (zero tail included), else the batch."""
    from kdcc_amd import nn_hip
    ld = getattr(batch, nn_hip._PADDED, 0)
    if not ld:
        return batch
    B = batch.shape[0]
    return batch.permute(0, 2, 3, 1).as_strided((B, 32, 32, ld), (1024 * ld, 32 * ld, ld, 1))


def vec_name(dtype, layout, vec=True):
    d, w = ("f32", 4) if dtype == torch.float32 else ("bf16", 8)
    return f"cifar_batch_kernel<{d},{'nchw' if layout == 'nchw' else 'nhwc'},{w if vec else 1}>"


# ---------------------------------------------------------------------------------------------- the kernel against the host path
@gpu
@pytest.mark.parametrize("B", [1, 5, 128])
@pytest.mark.parametrize("n", [37, 300])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_device_batches_equal_the_host_path_and_the_oracle(sets, dt, layout, n, B):
    from kdcc_amd import _lib, nn_hip
    dtype = DTYPES[dt]
    root, imgs, labels = sets[n]
    table = R.extreme_params(n, max(B, 18))                    # B = 128 on 37 images: the indices repeat
    dev, host = loader(root, B, "cuda", dtype=dtype, layout=layout), loader(root, B, "cpu", dtype=dtype, layout=layout)
    got, want = list(dev.batches(table)), list(host.batches(table))
    assert _lib.last_plumbing_kernel() == vec_name(dtype, layout), "a loader's own buffers take the 16-byte stores"
    assert len(got) == len(want) == -(-len(table) // B)
    for (x, t), (hx, ht) in zip(got, want):
        assert x.is_cuda and t.is_cuda and x.dtype == dtype and t.dtype == torch.int64
        assert x.shape == hx.shape and x.stride() == hx.stride() and getattr(x, nn_hip._PADDED, 0) == getattr(hx, nn_hip._PADDED, 0)
        assert torch.equal(whole(x).cpu(), whole(hx)), "the batch, and for `padded` every byte of its zero tail"
        assert torch.equal(t.cpu(), ht)
    ox, oy = R.oracle_batch(imgs, labels, table, R.C100_MEAN, R.C100_STD, dtype)
    assert torch.equal(torch.cat([R.logical(x.cpu()) for x, _ in got]), ox) and torch.equal(torch.cat([t.cpu() for _, t in got]), oy)


_DIRECT = {}


def direct_reference(sets, dt):
    """(table, oracle batch (B,3,32,32) dense, labels), computed once per dtype: 45 rows on the 37-image set (B odd: ld = 5 and 3 make
    element counts whose 16-byte pieces straddle pixels and images)."""
    if dt not in _DIRECT:
        _, imgs, labels = sets[37]
        table = R.extreme_params(37, 45)
        _DIRECT[dt] = (table,) + R.oracle_batch(imgs, labels, table, R.C100_MEAN, R.C100_STD, DTYPES[dt])
    return _DIRECT[dt]


@gpu
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("ld", [0, 3, 5, 8, 32, 64], ids=lambda v: "nchw" if v == 0 else f"ld{v}")
@pytest.mark.parametrize("offset", [0, 1, 4], ids=lambda v: f"off{v}")
def test_the_op_on_garbage_filled_views_vector_and_scalar(sets, dt, ld, offset):
    """ops.cifar_batch into storage full of NaN patterns: a dense `out` (and any 16-byte aligned base) takes the vector kernel; the
    channel prefix of a wider buffer one element (2 or 4 bytes) off takes the scalar one.  Either way the kernel writes the whole
    pixel stride -- zeros behind channel 3 -- and nothing in front of or behind the view.  ld = 0 stands for dense NCHW."""
    from kdcc_amd import _lib, ops
    from kdcc_amd.base.base_data_loader import normalisation_table
    dtype = DTYPES[dt]
    root, imgs, labels = sets[37]
    table, ref, ref_y = direct_reference(sets, dt)
    B = table.shape[0]
    es = torch.empty((), dtype=dtype).element_size()
    elems = B * 1024 * (ld or 3)
    guard = 64
    flat = torch.full((elems + 2 * guard,), float("nan"), dtype=dtype, device="cuda")
    region = flat[guard + offset: guard + offset + elems]
    aligned = (region.data_ptr() % 16) == 0
    assert aligned == (offset * es % 16 == 0)
    if ld == 0:
        out = region.view(B, 3, 32, 32)
    else:
        out = region.view(B, 32, 32, ld)[..., :3].permute(0, 3, 1, 2)
    data = torch.from_numpy(imgs).cuda()
    lab = torch.tensor(labels, dtype=torch.int64, device="cuda")
    tab = normalisation_table(R.C100_MEAN, R.C100_STD, dtype).cuda()
    y = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    got, got_y = ops.cifar_batch(data, lab, table.cuda(), tab, out, y)
    assert _lib.last_plumbing_kernel() == vec_name(dtype, "nchw" if ld == 0 else "nhwc", vec=aligned)
    assert got is out and got_y is y and torch.equal(y.cpu(), ref_y)
    assert torch.equal(out.cpu().contiguous(), ref)
    if ld > 3:
        tail = region.view(B, 32, 32, ld)[..., 3:]
        assert tail.numel() == B * 1024 * (ld - 3) and not bool(tail.view(torch.int16 if es == 2 else torch.int32).any()), "the zero tail, bit for bit"
    assert bool(flat[:guard + offset].isnan().all()) and bool(flat[guard + offset + elems:].isnan().all()), "nothing outside the view is written"


@gpu
def test_the_wrapper_refuses_what_it_must_without_a_launch(sets):
    from kdcc_amd import _lib, ops
    from kdcc_amd.base.base_data_loader import normalisation_table
    _, imgs, labels = sets[37]
    data, lab = torch.from_numpy(imgs).cuda(), torch.tensor(labels, dtype=torch.int64, device="cuda")
    tab = normalisation_table(R.C100_MEAN, R.C100_STD).cuda()
    out = torch.full((2, 3, 32, 32), 5.0, device="cuda")
    ops.cifar_batch(data, lab, torch.tensor([[0, 4, 4, 0], [36, 0, 8, 1]], dtype=torch.int32).cuda(), tab, out)
    before = out.clone()
    for bad in ([37, 4, 4, 0], [-1, 4, 4, 0], [2 ** 31 - 1, 4, 4, 0], [0, 9, 4, 0], [0, 4, -1, 0], [0, 4, 4, 2]):
        for where in ("cuda", "cpu"):
            with pytest.raises((ValueError, _lib.KdccError)) as e:
                ops.cifar_batch(data, lab, torch.tensor([[1, 4, 4, 0], bad], dtype=torch.int32).to(where), tab, out)
            assert (e.type is ValueError) == (where == "cuda"), "an out-of-range table is a ValueError; a host table is no operand at all"
    torch.cuda.synchronize()
    assert torch.equal(out, before), "a refused call launches nothing"
    ok = torch.tensor([[0, 4, 4, 0], [1, 4, 4, 0]], dtype=torch.int32).cuda()
    for kw, exc in ((dict(table=tab.to(BF)), ValueError), (dict(table=tab[:, :255]), ValueError), (dict(out=out[:1]), ValueError),
                    (dict(out=out.double()), TypeError), (dict(data=data.permute(0, 3, 1, 2)), ValueError), (dict(labels=lab.int()), ValueError),
                    (dict(params=ok.long()), ValueError), (dict(out=out.cpu()), _lib.KdccError)):
        args = dict(data=data, labels=lab, params=ok, table=tab, out=out)
        args.update(kw)
        with pytest.raises(exc):
            ops.cifar_batch(**args)
    with pytest.raises(ValueError):
        loader(sets[37][0], 5, "cuda").batches(torch.tensor([[37, 4, 4, 0]], dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------ whole epochs
@gpu
@pytest.mark.parametrize("layout,dt", [("nchw", "fp32"), ("padded", "bf16")])
def test_a_whole_epoch_equals_the_same_seed_host_loader(sets, layout, dt):
    root = sets[37][0]
    kw = dict(dtype=DTYPES[dt], layout=layout, seed=5, validation_split=0.0)
    dev, host = loader(root, 5, "cuda", **kw), loader(root, 5, "cpu", **kw)
    for epoch in range(2):
        got, want = list(dev), list(host)
        assert torch.equal(dev.epoch_params(), host.epoch_params())
        assert [x.shape[0] for x, _ in got] == [5] * 7 + [2] == [x.shape[0] for x, _ in want], "the short last batch"
        for (x, t), (hx, ht) in zip(got, want):
            assert torch.equal(whole(x).cpu(), whole(hx)) and torch.equal(t.cpu(), ht)
    V, HV = loader(root, 5, "cuda", **{**kw, "validation_split": 0.3}).split_validation(), loader(root, 5, "cpu", **{**kw, "validation_split": 0.3}).split_validation()
    for (x, t), (hx, ht) in zip(list(V), list(HV)):
        assert torch.equal(whole(x).cpu(), whole(hx)) and torch.equal(t.cpu(), ht)
    assert V.n_samples == HV.n_samples == 11


@gpu
def test_a_batch_made_on_a_side_stream_is_whole_after_that_streams_sync(sets):
    root = sets[300][0]
    dev, host = loader(root, 128, "cuda", dtype=BF, layout="padded", seed=9), loader(root, 128, "cpu", dtype=BF, layout="padded", seed=9)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = list(dev)
    side.synchronize()
    for (x, t), (hx, ht) in zip(got, list(host)):
        assert torch.equal(whole(x).cpu(), whole(hx)) and torch.equal(t.cpu(), ht)


# ------------------------------------------------------------------------------------------- the students read it in place
@gpu
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_a_padded_batch_reaches_the_stem_conv_without_a_padding_copy(sets, monkeypatch, dt):
    """Teacher + student forward of a depth-10 widen-4 Wide-ResNet: the stem conv of each pads a plain channels-last batch (2 copies);
    a "padded" batch of the same values it reads in place (0), to the same logits bit for bit.  G = 64 in bf16, 32 in fp32."""
    from kdcc_amd import nn_hip
    from kdcc_amd.models import cifar_models
    from kdcc_amd.models.students import DepthwiseStudent
    dtype = DTYPES[dt]
    G = 64 if dtype == BF else 32
    copies = []
    orig = nn_hip._nhwc_padded
    monkeypatch.setattr(nn_hip, "_nhwc_padded", lambda t, cpad: (copies.append((t.shape[1], cpad)), orig(t, cpad))[1])
    teacher = seeded_fill_(cifar_models.wrn(**SMALL), "wrn.").cuda().eval()
    model = DepthwiseStudent(teacher, None, dtype=BF) if dtype == BF else DepthwiseStudent(teacher, None)
    assert model.module_dtype == dtype
    model.eval()
    x, _ = next(iter(loader(sets[64][0], 16, "cuda", dtype=dtype, layout="padded", seed=3)))
    assert getattr(x, nn_hip._PADDED) == G == nn_hip._granule_up(3, dtype)
    plain = x.contiguous(memory_format=torch.channels_last)
    assert getattr(plain, nn_hip._PADDED, 0) == 0 and torch.equal(plain, x)
    with torch.no_grad():
        assert model._module_graph_batch(x) is x and model._module_graph_batch(plain) is plain
        s, t = model(x)
        assert copies == [], f"a padded batch was copied: {copies}"
        s2, t2 = model(plain)
        assert copies == [(3, G)] * 2, copies
    assert torch.equal(s, s2) and torch.equal(t, t2) and torch.equal(s, t) and bool(s.isfinite().all())


# ------------------------------------------------------------------------------------------------------ ClassificationTrainer
def wrn_config(root, save_dir):
    """tests/test_wrn_bf16_gpu.py's bf16 plan c1, epoch-based (no trainer.len_epoch), with the reference's loader block."""
    name = "block3.layer.0"
    cfg = trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir, dtype="bf16")
    cfg.update(name="cifar_loader", teacher={"type": "wrn", "args": dict(SMALL)}, optimizer={"type": "SGD", "args": {"lr": 0.1}},
               kd_loss={"type": "KLDivergenceLoss", "args": {"temperature": 5}},
               hint_loss={"type": "MSELoss", "args": {"reduction": "mean", "num_classes": 1}}, metrics=["accuracy", "top_k_acc"],
               lr_scheduler={"type": "MultiStepLR", "args": {"milestones": [15, 25], "gamma": 0.2}},
               train_data_loader={"type": "Cifar100Dataloader", "args": {"data_dir": root, "batch_size": 16, "shuffle": True, "validation_split": 0.0,
                                                                         "num_workers": 0}})
    cfg["trainer"]["name"] = "ClassificationTrainer"
    del cfg["trainer"]["len_epoch"]
    cfg["pruning"] = {"args": {"dilation": 1, "padding": 1, "kernel_size": 3}, "hint": [{"name": name, "epoch": 1}],
                      "unfreeze": [{"name": name, "epoch": 1}], "pruning_plan": [{"name": name + ".conv2", "epoch": 1}]}
    return cfg


def run_epoch(root, save_dir, run_id, as_list):
    import kdcc_amd
    from kdcc_amd import ConfigParser, losses
    from kdcc_amd.models import cifar_models, metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer import ClassificationTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    config = ConfigParser(wrn_config(root, save_dir), run_id=run_id)
    feed = config.init_obj("train_data_loader", kdcc_amd.data_loader, dtype=BF, layout="padded", seed=21)
    assert feed.device.type == "cuda" and len(feed) == 4 and feed.n_samples == 64
    if as_list:
        feed = list(feed)
        assert len(feed) == 4 and all(x.shape[0] == 16 for x, _ in feed)
    teacher = seeded_fill_(config.init_obj("teacher", cifar_models), "wrn.").cuda().eval()
    model = DepthwiseStudent(teacher, config)
    assert model.module_dtype == BF
    orig_replace = model.replace

    def replace_and_seed(blocks, **kw):
        orig_replace(blocks, **kw)
        for b in blocks:
            seeded_fill_(model.get_block(b["name"], model.student), f"wrn.student.{b['name']}.")
    model.replace = replace_and_seed
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    metrics = [getattr(metric, m) for m in config["metrics"]]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    tr = ClassificationTrainer(model, crit, metrics, opt, config, feed, None, sched, WeightScheduler(config["weight_scheduler"]))
    assert tr.len_epoch == 4
    return tr._train_epoch(1)


@gpu
def test_a_trainer_epoch_fed_by_the_loader_logs_what_a_list_of_its_batches_logs(sets, tmp_path):
    root = sets[64][0]
    a = run_epoch(root, str(tmp_path / "a"), "loader", as_list=False)
    b = run_epoch(root, str(tmp_path / "b"), "list", as_list=True)
    for k in LOSSES:
        assert a[k] == b[k] and a[k] == a[k], f"{k}: {a[k]} fed by the loader, {b[k]} fed by the list"
