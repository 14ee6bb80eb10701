#!/usr/bin/env python3
"""Measure the class-uniform Cityscapes loader (kdcc_amd.data_loader.CityscapesUniformDataloader): its centroid pass
(kd_seg_class_stats) against the HBM rate and against two host computations of the same centroids, its construction and its batches
against CityscapesDataloader.  Timing only; nothing here is asserted.  One measurement per process: run each step as a fresh
process under a time limit of its own and alternate the two sides of a comparison (profiles/cityscapes_uniform.md has the commands).

    python tools/bench_cityscapes_uniform.py --mode stats      [--images 64] [--tile 1024] [--labels blocks|noise] [--reps 20]
    python tools/bench_cityscapes_uniform.py --mode host-stats [--images 64] [--tile 1024] [--labels ...]
    python tools/bench_cityscapes_uniform.py --mode host-ref   [--images 64] [--tile 1024] [--labels ...]
    python tools/bench_cityscapes_uniform.py --mode make      --data-dir DIR [--images 40]    (write the synthetic tree once)
    python tools/bench_cityscapes_uniform.py --mode construct --data-dir DIR --which uniform|plain
    python tools/bench_cityscapes_uniform.py --mode loader    --data-dir DIR --which uniform|plain [--epochs 3]

--mode stats: HIP-event time of ops.seg_class_stats over (images, 1024, 2048) synthetic train-id maps generated on the device, median
  of --reps after 3 warm-up calls; the bytes are the labels read plus the statistics cleared and written.
--mode host-stats: the host path of ops.seg_class_stats (torch integer ops) on the same maps copied to the host, wall clock.
--mode host-ref: the reference's per-image chain as the library calls it makes (data_loader/uniform.py of the reference: PIL decode of
  the label PNG, 34 masked assignments for the id remap, scipy.ndimage.center_of_mass per tile and present class), one image after
  the other (the reference runs it on 32 threads), on the same maps written as label-id PNGs; says so when scipy is missing.
--mode construct / loader: construction wall clock, and wall clock per batch as tools/bench_cityscapes_loader.py --mode loader takes
  it (source 1024 x 2048, crop 512, batch 4, jitter and blur on), of either loader on one synthetic tree.
Labels: `blocks` are 32 x 32 blocks of one id (runs, as label maps have them); `noise` changes at every pixel (the worst case for
the kernel's run accumulation).  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 1024, 2048
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12       # MI355X: float4 copy measured, and the specification


def device_ids(a):
    """Label ids 0..33 (n, H, W) uint8 on the device, from a seed."""
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    if a.labels == "noise":
        return torch.randint(0, 34, (a.images, H, W), generator=g, device="cuda", dtype=torch.uint8)
    small = torch.randint(0, 34, (a.images, H // 32, W // 32), generator=g, device="cuda", dtype=torch.uint8)
    return small.repeat_interleave(32, 1).repeat_interleave(32, 2).contiguous()


def train_ids(ids):
    """The loader's id -> train id remap, 64 maps at a time (the index is int64)."""
    from kdcc_amd.data_loader.cityscapes import _lut
    lut = torch.from_numpy(_lut()).to(ids.device)
    return torch.cat([lut[c.long()] for c in ids.split(64)])


def mode_stats(a):
    from kdcc_amd import _lib, ops
    t = train_ids(device_ids(a))
    for _ in range(3):
        out = ops.seg_class_stats(t, a.tile)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(a.reps):
        start.record()
        ops.seg_class_stats(t, a.tile)
        end.record()
        end.synchronize()
        us.append(start.elapsed_time(end) * 1e3)
    med = float(np.median(us))
    nbytes = t.numel() + 2 * out.numel() * 8
    return dict(kernel=_lib.last_plumbing_kernel(), shape=list(t.shape), us=med, us_min=min(us), us_max=max(us), bytes=nbytes,
                TBps=nbytes / med / 1e6, share_of_measured_hbm=nbytes / (med * 1e-6) / HBM_MEASURED, share_of_spec_hbm=nbytes / (med * 1e-6) / HBM_SPEC,
                note="the time includes the clearing of stats (one memset in front of the kernel)")


def mode_host_stats(a):
    from kdcc_amd import ops
    t = train_ids(device_ids(a)).cpu()
    ops.seg_class_stats(t[:2], a.tile)
    t0 = time.perf_counter()
    ops.seg_class_stats(t, a.tile)
    s = time.perf_counter() - t0
    return dict(shape=list(t.shape), seconds=s, ms_per_image=s / len(t) * 1e3, threads=torch.get_num_threads())


def mode_host_ref(a):
    try:
        from scipy import ndimage
    except ImportError:
        return dict(skipped="scipy is not installed here")
    from PIL import Image
    from kdcc_amd.data_loader.cityscapes import ID_TO_TRAINID
    ids = device_ids(a).cpu().numpy()
    with tempfile.TemporaryDirectory() as root:
        files = []
        for i, m in enumerate(ids):
            files.append(os.path.join(root, f"{i:06d}_gtFine_labelIds.png"))
            Image.fromarray(m).save(files[-1], compress_level=1)
        t0 = time.perf_counter()
        found = 0
        for f in files:
            mask = np.array(Image.open(f))
            copy = mask.copy()
            for k, v in ID_TO_TRAINID.items():
                mask[copy == k] = v
            for y in range(mask.shape[0] // a.tile):
                for x in range(mask.shape[1] // a.tile):
                    patch = mask[y * a.tile:(y + 1) * a.tile, x * a.tile:(x + 1) * a.tile]
                    for c in range(19):
                        if c in patch:
                            cy, cx = ndimage.center_of_mass((patch == c).astype(int))
                            found += 1
        s = time.perf_counter() - t0
    return dict(images=len(files), centroids=found, seconds=s, ms_per_image=s / len(files) * 1e3, note="serial; the reference maps it over 32 threads")


def loader_of(a):
    from kdcc_amd import data_loader
    import bench_cityscapes_loader as B
    _, tr, _ = B.transforms()
    cls = data_loader.CityscapesUniformDataloader if a.which == "uniform" else data_loader.CityscapesDataloader
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loader = cls(a.data_dir, 4, shuffle=True, split="train", device="cuda", seed=0, **tr)
    torch.cuda.synchronize()
    return loader, time.perf_counter() - t0


def mode_construct(a):
    torch.zeros(1, device="cuda")       # the context, not the loader
    loader, s = loader_of(a)
    return dict(which=a.which, images=len(loader.dataset), samples=loader.n_samples, seconds=s)


def mode_loader(a):
    loader, _ = loader_of(a)
    times = []
    for _ in range(a.epochs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for x, t in loader:
            pass
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / len(loader))
    per = float(np.median(times[1:]))
    centred = int(loader.imgs_uniform[:, 1].sum()) if a.which == "uniform" else 0
    return dict(which=a.which, batches=len(loader), centred_entries=centred, shape=list(x.shape), us_per_batch=per * 1e6,
                epochs_us=[t * 1e6 for t in times])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", required=True, choices=["stats", "host-stats", "host-ref", "make", "construct", "loader"])
    p.add_argument("--images", type=int, default=None)
    p.add_argument("--tile", type=int, default=1024)
    p.add_argument("--labels", default="blocks", choices=["blocks", "noise"])
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--which", default="uniform", choices=["uniform", "plain"])
    p.add_argument("--epochs", type=int, default=3)
    p.add_argument("--data-dir", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cityscapes_uniform.py measures on the GPU: none found")
    if a.mode in ("make", "construct", "loader"):
        if a.data_dir is None:
            raise SystemExit(f"--mode {a.mode} needs --data-dir")
        if a.mode == "make":
            import bench_cityscapes_loader as B
            B.synthetic_tree(a.data_dir, a.images or 40)
            print(json.dumps(dict(mode="make", data_dir=a.data_dir, images=a.images or 40)))
            return
    a.images = a.images or 64
    res = dict(mode=a.mode, labels=a.labels, tile=a.tile)
    res.update({"stats": mode_stats, "host-stats": mode_host_stats, "host-ref": mode_host_ref, "construct": mode_construct,
                "loader": mode_loader}[a.mode](a))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
