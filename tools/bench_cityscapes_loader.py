#!/usr/bin/env python3
"""Measure the device-resident Cityscapes loader (kdcc_amd.data_loader.CityscapesDataloader) against a host composition of the
reference's pipeline.  Timing only; nothing here is asserted.

    python tools/bench_cityscapes_loader.py --mode loader [--dtype fp32|bf16] [--layout nchw|nhwc|padded]
    python tools/bench_cityscapes_loader.py --mode val    [--dtype ...] [--layout ...]
    python tools/bench_cityscapes_loader.py --mode stages
    python tools/bench_cityscapes_loader.py --mode host   [--host-images 8]
    python tools/bench_cityscapes_loader.py --mode make --data-dir DIR      (write the synthetic tree once, for later calls)
    python tools/bench_cityscapes_loader.py --mode epoch --feed loader|synthetic
    [--images 12] [--data-dir DIR]

--mode loader: training batches at the shipped shape (source 1024x2048, crop 512, batch 4, colour jitter 0.2, Gaussian blur): wall
  clock per batch over --epochs epochs of the synthetic set with one synchronisation at the end of each, the first not counted.  This
  includes the host's per-batch table computation and upload.
--mode val: 8 full-size images, augmentation off, one batch of 8: the gather straight from the resident bytes.
--mode stages: HIP-event time of each launch (crop, jitter, finish; the full-size gather) on prepared tables, with the bytes each
  must move and the rate that makes.
--mode host: the reference's chain per image with num_workers 0, as the library calls it makes (PIL resize / expand / crop /
  transpose, ImageEnhance and the HSV round trip, scipy.ndimage.gaussian_filter in float64, ToTensor / Normalize in torch), stacked
  and copied to the device.  skimage and torchvision are not installed, so this is their arithmetic, not their code.
--mode epoch: one LayerwiseTrainer epoch (len_epoch 100) of the shipped 51M_deeplab_all plan (random teacher, no snapshot, bf16),
  fed by the loader or by pre-made synthetic batches of the same shape.

The dataset is synthetic PNGs (smooth gradients plus noise, random label ids) written by this tool to a temporary directory unless
--data-dir names a tree.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG = os.path.join(ROOT, "tests", "golden", "cfg", "cityscapes", "51M_deeplab_all.json")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def synthetic_tree(root, n, H=1024, W=2048):
    from PIL import Image
    rng = np.random.default_rng(0)
    for split, m in (("train", n), ("val", 8)):
        for sub in ("leftImg8bit", "gtFine"):
            os.makedirs(os.path.join(root, sub, split, "synth"), exist_ok=True)
        for i in range(m):
            yy, xx = np.mgrid[0:H, 0:W]
            base = np.stack([(xx + 37 * i) % 256, (yy * 2 + 11 * i) % 256, ((xx + yy) // 3) % 256], -1)
            img = np.clip(base + rng.integers(-20, 21, size=(H, W, 3)), 0, 255).astype(np.uint8)
            ids = np.repeat(np.repeat(rng.integers(0, 34, size=(H // 32, W // 32)), 32, 0), 32, 1).astype(np.uint8)
            stem = f"synth_{i:06d}_000019"
            Image.fromarray(img).save(os.path.join(root, "leftImg8bit", split, "synth", stem + "_leftImg8bit.png"), compress_level=1)
            Image.fromarray(ids).save(os.path.join(root, "gtFine", split, "synth", stem + "_gtFine_labelIds.png"), compress_level=1)


def transforms():
    from kdcc_amd import data_loader
    with open(CFG) as f:
        cfg = json.load(f)
    joint, image, target, val = data_loader._create_transform(cfg)
    return cfg, dict(transforms=joint, transform=image, target_transform=target), dict(transform=val, target_transform=target)


def make_loader(a, train=True, batch=None):
    from kdcc_amd import data_loader
    cfg, tr, val = transforms()
    kw = dict(device="cuda", dtype=DTYPES[a.dtype], layout=a.layout, seed=0)
    if train:
        return data_loader.CityscapesDataloader(a.data_dir, batch or 4, shuffle=True, split="train", **tr, **kw)
    return data_loader.CityscapesDataloader(a.data_dir, batch or 8, shuffle=False, split="val", **val, **kw)


def mode_loader(a, train=True):
    loader = make_loader(a, train)
    times = []
    for _ in range(a.epochs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for x, t in loader:
            pass
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / len(loader))
    per = float(np.median(times[1:]))
    return dict(batch=loader.batch_size, shape=list(x.shape), us_per_batch=per * 1e6, batches_per_s=1.0 / per, img_per_s=loader.batch_size / per,
                epochs_us=[t * 1e6 for t in times])


def _event_us(fn, reps=20):
    for _ in range(3):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        start.record()
        fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end) * 1e3)
    return float(np.median(out))


def mode_stages(a):
    from kdcc_amd import ops
    from kdcc_amd.data_loader import seg_tables
    res = {}
    for dt in ("fp32", "bf16"):
        a.dtype = dt
        loader = make_loader(a, True)
        rows = loader._draw_epoch()[:4]
        tab, S = loader._expanded(rows)
        tab = tab.cuda()
        es = 4 if dt == "fp32" else 2
        B = 4
        img, msk = ops.seg_crop(loader._data, loader._targets, tab, S, validated=True)
        if dt == "fp32":
            us = _event_us(lambda: ops.seg_crop(loader._data, loader._targets, tab, S, img, msk, validated=True))
            # the source window of each crop (3 image bytes and a label byte a pixel), the crop written, the table read
            src = sum(min(S, r[1]) * loader.W / r[1] * min(S, r[2]) * loader.H / r[2] * 4 for r in rows.tolist())
            nbytes = float(src) + B * S * S * 4 + tab.numel() * 4
            res["crop"] = dict(us=us, bytes=nbytes, GBps=nbytes / us / 1e3)
            ws = torch.empty(64, dtype=torch.uint8, device="cuda")
            us = _event_us(lambda: ops.seg_jitter(img, tab, ws, validated=True))
            nbytes = B * S * S * 3 * (2 + 2)
            res["jitter"] = dict(us=us, bytes=nbytes, GBps=nbytes / us / 1e3, note="two passes, each a read and a write at most")
        out, _ = loader._new_out(B, S, S)
        mo = torch.empty((B, S, S), dtype=torch.int64, device="cuda")
        for blur in (True, False):
            us = _event_us(lambda: ops.seg_finish(img, msk, tab, loader._table, out, mo, blur=blur, validated=True))
            nbytes = B * S * S * (4 + 3 * es + 8)
            res[f"finish_{'blur' if blur else 'gather'}_{dt}_{a.layout}"] = dict(us=us, bytes=nbytes, GBps=nbytes / us / 1e3)
        val = make_loader(a, False)
        vrows = val._draw_epoch().cuda()
        vout, _ = val._new_out(8, val.H, val.W)
        vmo = torch.empty((8, val.H, val.W), dtype=torch.int64, device="cuda")
        us = _event_us(lambda: ops.seg_finish(val._data, val._targets, vrows, val._table, vout, vmo, use_index=True, validated=True))
        nbytes = 8 * val.H * val.W * (4 + 3 * es + 8)
        res[f"full_size_gather_{dt}_{a.layout}"] = dict(us=us, bytes=nbytes, GBps=nbytes / us / 1e3)
    return res


def mode_host(a):
    import _cityscapes_loader_ref as R
    from kdcc_amd.data_loader import seg_tables
    from kdcc_amd.data_loader.cityscapes import CityscapesArrays
    cfg, tr, _ = transforms()
    ds = CityscapesArrays(a.data_dir, "train")
    H, W = ds.data.shape[1:3]
    spec = dict(crop=512, scale_min=0.5, scale_max=2.0, flip=True, color_aug=0.2, blur=True)
    g = torch.Generator()
    g.manual_seed(0)
    rows = seg_tables.draw_rows(np.arange(a.host_images) % len(ds), W, H, spec, g).numpy()
    t0 = time.perf_counter()
    for s in range(0, len(rows), 4):
        xs, ts = zip(*[R.ref_sample(ds.data[r[0]], ds.targets[r[0]], r, 512) for r in rows[s:s + 4]])
        x, t = torch.stack(xs).cuda(), torch.stack(ts).cuda()
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / (len(rows) / 4)
    return dict(images=len(rows), us_per_batch=per * 1e6, batches_per_s=1.0 / per, img_per_s=4 / per)


def mode_epoch(a):
    from kdcc_amd import ConfigParser, losses, models
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer import LayerwiseTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    with open(CFG) as f:
        cfg = json.load(f)
    cfg["teacher"].pop("snapshot", None)
    cfg["trainer"].update(save_dir=tempfile.mkdtemp(), verbosity=0, tensorboard=False, monitor="off", len_epoch=a.len_epoch, dtype="bf16",
                          log_step=1000, save_period=1000)
    cfg["metrics"] = []
    config = ConfigParser(cfg, run_id="bench")
    torch.manual_seed(0)
    teacher = config.init_obj("teacher", models).eval()
    model = DepthwiseStudent(teacher, config)
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    if a.feed == "loader":
        feed = make_loader(a, True)
    else:
        gen = torch.Generator().manual_seed(0)
        feed = [(torch.randn(4, 3, 512, 512, generator=gen).cuda(), torch.randint(0, 19, (4, 512, 512), generator=gen).cuda()) for _ in range(3)]

    class Cycle:        # len_epoch batches from a short feed, as the reference's inf_loop
        def __init__(self, src, n):
            self.src, self.n, self.batch_size = src, n, 4

        def __len__(self):
            return self.n

        def __iter__(self):
            k = 0
            while k < self.n:
                for b in self.src:
                    if k >= self.n:
                        return
                    k += 1
                    yield b
    tr = LayerwiseTrainer(model, crit, [], opt, config, Cycle(feed, a.len_epoch), None, sched, WeightScheduler(config["weight_scheduler"]))
    times = []
    for epoch in (1, 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr._train_epoch(epoch)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return dict(feed=a.feed, len_epoch=a.len_epoch, epoch_s=times, ms_per_step=times[-1] / a.len_epoch * 1e3)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", required=True, choices=["make", "loader", "val", "stages", "host", "epoch"])
    p.add_argument("--dtype", default="fp32", choices=list(DTYPES))
    p.add_argument("--layout", default="nchw", choices=["nchw", "nhwc", "padded"])
    p.add_argument("--feed", default="loader", choices=["loader", "synthetic"])
    p.add_argument("--images", type=int, default=12)
    p.add_argument("--host-images", type=int, default=8)
    p.add_argument("--epochs", type=int, default=3)
    p.add_argument("--len-epoch", type=int, default=100)
    p.add_argument("--data-dir", default=None)
    a = p.parse_args()
    tmp = None
    if a.data_dir is None:
        tmp = tempfile.TemporaryDirectory()
        a.data_dir = tmp.name
        synthetic_tree(a.data_dir, a.images)
    if a.mode == "make":        # only write the synthetic tree into --data-dir, for several measuring processes to share
        synthetic_tree(a.data_dir, a.images)
        print(json.dumps(dict(mode="make", data_dir=a.data_dir, images=a.images)))
        return
    res = dict(mode=a.mode, dtype=a.dtype, layout=a.layout)
    res.update({"loader": lambda: mode_loader(a, True), "val": lambda: mode_loader(a, False), "stages": lambda: mode_stages(a),
                "host": lambda: mode_host(a), "epoch": lambda: mode_epoch(a)}[a.mode]())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
