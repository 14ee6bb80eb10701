#!/usr/bin/env python3
"""Measure the device-resident CIFAR loaders (kdcc_amd.data_loader) against a host restatement of the reference's pipeline.

    python tools/bench_cifar_loader.py --mode loader [--layout nchw|nhwc|padded|all] [--dtype fp32|bf16|all]
    python tools/bench_cifar_loader.py --mode host
    python tools/bench_cifar_loader.py --mode epoch --feed device|host
    [--images 12800] [--batch 128] [--epochs 3] [--data-dir DIR]

--mode loader: batches per second of Cifar100Dataloader on the GPU (training=True, shuffle), wall clock over whole epochs with one
  synchronisation at the end of each, the first epoch (warm-up) not counted; and the kernel's own time per batch from HIP events
  around one more epoch.
--mode host: the reference's pipeline with num_workers 0, restated: per image PIL pad / random crop / random flip (the calls
  torchvision's RandomCrop(32, padding=4) and RandomHorizontalFlip make), ToTensor and Normalize in torch, a stacked batch, then the
  H2D copy of batch and labels.  torchvision itself is not installed, so this is its arithmetic, not its code.
--mode epoch: one ClassificationTrainer epoch of the WRN-28-10 CIFAR-100 config 1 (tests/golden/cfg/cifar100/wrn_28_10/config1.json:
  random teacher, no snapshot) with trainer.dtype bf16, fed by the device loader in the "padded" bf16 layout or by the host
  pipeline; wall clock of the epoch, and the padding copies (nn_hip._nhwc_padded calls) of one more, untimed step.

Without --data-dir a synthetic dataset of --images random images is written to a temporary directory in the CIFAR-100 python
format.  Prints one JSON line."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


def synthetic_cifar100(root, n):
    base = os.path.join(root, "cifar-100-python")
    os.makedirs(base, exist_ok=True)
    rng = np.random.default_rng(0)
    for name, m in (("train", n), ("test", 128)):
        with open(os.path.join(base, name), "wb") as f:
            pickle.dump({"data": rng.integers(0, 256, size=(m, 3072), dtype=np.uint8), "fine_labels": [int(v) for v in rng.integers(0, 100, size=m)]}, f)


class HostPipeline:
    """The reference's loader with num_workers 0, restated: one PIL image at a time on the host, batches of host tensors."""

    def __init__(self, data, targets, batch):
        self.data, self.targets, self.batch_size = data, targets, batch
        self.mean, self.std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)

    def __len__(self):
        return -(-len(self.data) // self.batch_size)

    def one(self, i):
        from PIL import Image, ImageOps
        img = ImageOps.expand(Image.fromarray(self.data[i]), border=4, fill=0)
        dy, dx = int(torch.randint(0, 9, (1,)).item()), int(torch.randint(0, 9, (1,)).item())
        img = img.crop((dx, dy, dx + 32, dy + 32))
        if torch.rand(1) < 0.5:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        t = torch.from_numpy(np.array(img, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        return t.sub_(self.mean).div_(self.std)

    def __iter__(self):
        order = torch.randperm(len(self.data)).tolist()
        for s in range(0, len(order), self.batch_size):
            idx = order[s:s + self.batch_size]
            yield torch.stack([self.one(i) for i in idx]), torch.tensor([self.targets[i] for i in idx], dtype=torch.int64)


def time_epochs(feed, epochs, to_device):
    """Batches per second over `epochs` epochs after one warm-up epoch; a synchronisation ends each epoch."""
    n, dt = 0, 0.0
    for e in range(epochs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        for x, y in feed:
            if to_device:
                x, y = x.cuda(), y.cuda()
            k += 1
        torch.cuda.synchronize()
        if e > 0:
            n, dt = n + k, dt + time.perf_counter() - t0
    return n / dt, 1e3 * dt / n


class Timed:
    """The feed, with the host clock read (behind a synchronisation) when batch `warm` is asked for: the steps before it load code
    objects and pack weights."""

    def __init__(self, feed, warm):
        self.feed, self.warm, self.t0 = feed, warm, None

    def __len__(self):
        return len(self.feed)

    def __iter__(self):
        it = iter(self.feed)
        for i in range(len(self.feed)):
            if i == self.warm:
                torch.cuda.synchronize()
                self.t0 = time.perf_counter()
            yield next(it)


def run_epoch(feed, root, warm=10):
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ConfigParser, losses, nn_hip
    from kdcc_amd.models import cifar_models, metric
    from kdcc_amd.models.students import DepthwiseStudent
    from kdcc_amd.trainer import ClassificationTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg", "cifar100", "wrn_28_10", "config1.json")))
    cfg["teacher"].pop("snapshot", None)
    cfg["trainer"].update(save_dir=os.path.join(root, "saved"), tensorboard=False, verbosity=0, dtype="bf16", log_step=10 ** 9)
    config = ConfigParser(cfg, run_id="bench")
    torch.manual_seed(0)
    teacher = config.init_obj("teacher", cifar_models).cuda().eval()
    model = DepthwiseStudent(teacher, config)
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    timed = Timed(feed, warm)
    tr = ClassificationTrainer(model, crit, [getattr(metric, m) for m in config["metrics"]], opt, config, timed, None, sched,
                               WeightScheduler(config["weight_scheduler"]))
    log = tr._train_epoch(1)
    torch.cuda.synchronize()
    wall = time.perf_counter() - timed.t0
    copies, pad = [], nn_hip._nhwc_padded
    nn_hip._nhwc_padded = lambda t, cpad: (copies.append(f"{t.shape[1]}->{cpad}"), pad(t, cpad))[1]
    try:
        x, y = next(iter(feed))
        s, t = model(x.cuda())
        crit[1](s, t).backward()
        torch.cuda.synchronize()
    finally:
        nn_hip._nhwc_padded = pad
    steps = len(feed) - warm
    return {"timed_wall_s": round(wall, 3), "timed_steps": steps, "warmup_steps": warm, "ms_per_step": round(1e3 * wall / steps, 3), "kd_loss": log["kd_loss"],
            "padding_copies_per_step": len(copies), "padding_copies": {k: copies.count(k) for k in sorted(set(copies))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loader", "host", "epoch"), required=True)
    ap.add_argument("--layout", choices=("nchw", "nhwc", "padded", "all"), default="all")
    ap.add_argument("--dtype", choices=("fp32", "bf16", "all"), default="all")
    ap.add_argument("--feed", choices=("device", "host"), default="device")
    ap.add_argument("--images", type=int, default=12800)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--data-dir", default=None)
    a = ap.parse_args()
    import kdcc_amd  # noqa: F401
    from kdcc_amd import data_loader
    tmp = tempfile.TemporaryDirectory()
    root = a.data_dir or tmp.name
    if a.data_dir is None:
        synthetic_cifar100(root, a.images)
    torch.manual_seed(0)
    out = {"tool": "bench_cifar_loader", "mode": a.mode, "batch": a.batch}
    if a.mode == "loader":
        for layout in (("nchw", "nhwc", "padded") if a.layout == "all" else (a.layout,)):
            for dt in (("fp32", "bf16") if a.dtype == "all" else (a.dtype,)):
                L = data_loader.Cifar100Dataloader(root, a.batch, device="cuda", dtype=torch.bfloat16 if dt == "bf16" else torch.float32,
                                                   layout=layout, seed=0)
                bps, ms = time_epochs(L, a.epochs, False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                batches = L.batches(L._draw_epoch())          # the table is uploaded before the first event
                e0.record()
                for _ in batches:                             # (events around a whole epoch: launches and the gaps between them)
                    pass
                e1.record()
                torch.cuda.synchronize()
                print(json.dumps(dict(out, layout=layout, dtype=dt, images=L.n_samples, batches_per_s=round(bps, 1), ms_per_batch_wall=round(ms, 4),
                                      img_per_s=round(bps * a.batch, 0), us_per_batch_device=round(1e3 * e0.elapsed_time(e1) / len(L), 2))))
        return
    elif a.mode == "host":
        ds = data_loader.data_loaders.CifarArrays(root, "cifar-100-python", ["train"], "fine_labels")
        bps, ms = time_epochs(HostPipeline(ds.data, ds.targets, a.batch), a.epochs, True)
        out.update(images=len(ds), batches_per_s=round(bps, 1), ms_per_batch_wall=round(ms, 4), img_per_s=round(bps * a.batch, 0),
                   cpus=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())
    else:
        if a.feed == "device":
            feed = data_loader.Cifar100Dataloader(root, a.batch, device="cuda", dtype=torch.bfloat16, layout="padded", seed=0)
        else:
            ds = data_loader.data_loaders.CifarArrays(root, "cifar-100-python", ["train"], "fine_labels")
            feed = HostPipeline(ds.data, ds.targets, a.batch)
        out.update(feed=a.feed, images=a.images, **run_epoch(feed, root))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
