"""`Cifar10Dataloader` / `Cifar100Dataloader` (reference data_loader/data_loaders.py:8-53) over base.BaseDataLoader: the dataset read
from the standard python pickles (never downloaded, no torchvision), resident on the device, one kd_cifar_batch launch per batch.

The reference's constructor arguments come first and mean what they mean there (num_workers is accepted and ignored); then,
keyword-only: device (None: the current GPU if there is one, else the CPU), dtype (float32 / bfloat16), layout ("nchw" | "nhwc" |
"padded", see BaseDataLoader) and seed.  The normalisation constants are the reference's, its quirk included: the CIFAR-10 loader
normalises with the ImageNet statistics.  The random stream is not the reference's (see base/base_data_loader.py): torchvision draws
per image from the global RNG, these loaders draw a whole epoch at a time from their own generator.

`CityscapesDataloader` (reference data_loader/data_loaders.py:56-81) follows the same shape with its own dataset reader (cityscapes.py),
parameter table and host-tensor path (seg_tables.py) and kernels (csrc/seg_data_ops.hip); see its docstring.
`CityscapesUniformDataloader` (reference data_loader/data_loaders.py:83-97) is that loader over a class-uniform epoch list (uniform.py)."""
import os
import pickle

import numpy as np
import torch

from .. import nn_hip, ops
from ..base.base_data_loader import BaseDataLoader, LAYOUTS, normalisation_table
from . import joint_transforms, seg_tables, uniform
from . import transforms as extended_transforms
from .cityscapes import CityscapesArrays, ConcatArrays


class CifarArrays:
    """The images (n,32,32,3) uint8 and labels of a list of CIFAR python-format files (rows are planar R, G, B on disk)."""

    def __init__(self, root, folder, files, label_key):
        base = os.path.join(root, folder)
        if not os.path.isdir(base):
            raise FileNotFoundError(f"{base}: no such directory (the dataset is read from disk, never downloaded)")
        data, targets = [], []
        for name in files:
            path = os.path.join(base, name)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"{path}: missing dataset file")
            with open(path, "rb") as f:
                entry = pickle.load(f, encoding="latin1")
            data.append(np.asarray(entry["data"], dtype=np.uint8).reshape(-1, 3, 32, 32))
            targets.extend(int(t) for t in entry[label_key])
        self.data = np.ascontiguousarray(np.concatenate(data).transpose(0, 2, 3, 1))
        self.targets = targets
        if len(self.targets) != len(self.data) or len(self.data) == 0:
            raise ValueError(f"{base}: {len(self.data)} images, {len(self.targets)} labels")

    def __len__(self):
        return len(self.data)


class Cifar10Dataloader(BaseDataLoader):
    """CIFAR-10 from <data_dir>/cifar-10-batches-py/{data_batch_1..5 | test_batch}; ImageNet mean / std, as the reference."""
    MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def __init__(self, data_dir, batch_size, shuffle=True, validation_split=0.0, num_workers=1, training=True, *, device=None,
                 dtype=torch.float32, layout="nchw", seed=None):
        self.data_dir = data_dir
        files = [f"data_batch_{i}" for i in range(1, 6)] if training else ["test_batch"]
        dataset = CifarArrays(data_dir, "cifar-10-batches-py", files, "labels")
        super().__init__(dataset, batch_size, shuffle, validation_split, num_workers, mean=self.MEAN, std=self.STD, training=training,
                         device=device, dtype=dtype, layout=layout, seed=seed)


class Cifar100Dataloader(BaseDataLoader):
    """CIFAR-100 from <data_dir>/cifar-100-python/{train | test}, fine labels."""
    MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)

    def __init__(self, data_dir, batch_size, shuffle=True, validation_split=0.0, num_workers=1, training=True, *, device=None,
                 dtype=torch.float32, layout="nchw", seed=None):
        self.data_dir = data_dir
        dataset = CifarArrays(data_dir, "cifar-100-python", ["train" if training else "test"], "fine_labels")
        super().__init__(dataset, batch_size, shuffle, validation_split, num_workers, mean=self.MEAN, std=self.STD, training=training,
                         device=device, dtype=dtype, layout=layout, seed=seed)


def _refuse(item, why):
    raise ValueError(f"CityscapesDataloader: cannot express {item!r}: {why}")


def read_transform_spec(transforms, transform, target_transform):
    """(spec or None, mean, std) from the reference's three transform arguments (what `_create_transform` returns).  The loader runs
    one fixed chain -- RandomSizeAndCrop [, Resize(crop)] [, RandomHorizontallyFlip]; then on the image [ColorJitter(a, a, a, a)]
    [, RandomGaussianBlur], ToTensor, Normalize; MaskToTensor on the mask -- and refuses, by name, whatever is not that chain."""
    mean, std = Cityscapes_MEAN, Cityscapes_STD
    color_aug, blur = 0.0, False
    if transform is not None:
        items = list(getattr(transform, "transforms", None) or _refuse(transform, "the image transform must be a Compose"))
        stage = 0       # 0: before ColorJitter, 1: before the blur, 2: before ToTensor, 3: before Normalize, 4: done
        for it in items:
            if isinstance(it, extended_transforms.ColorJitter) and stage < 1:
                a = it.brightness
                if not (it.contrast == a and it.saturation == a and it.hue == a and 0 < a <= 0.5):
                    _refuse(it, "the four strengths must be one value in (0, 0.5]")
                color_aug, stage = float(a), 1
            elif isinstance(it, extended_transforms.RandomGaussianBlur) and stage < 2:
                blur, stage = True, 2
            elif isinstance(it, extended_transforms.ToTensor) and stage < 3:
                stage = 3
            elif isinstance(it, extended_transforms.Normalize) and stage == 3:
                mean, std, stage = it.mean, it.std, 4
            else:
                _refuse(it, "the image chain is [ColorJitter] [RandomGaussianBlur] ToTensor Normalize, in that order")
        if stage != 4:
            _refuse(transform, "the image chain must end with ToTensor, Normalize")
    if target_transform is not None and not isinstance(target_transform, extended_transforms.MaskToTensor):
        _refuse(target_transform, "the mask transform is MaskToTensor")
    if transforms is None:
        if color_aug > 0 or blur:
            _refuse(transform, "ColorJitter and RandomGaussianBlur run on the crop of RandomSizeAndCrop only")
        return None, mean, std
    items = list(getattr(transforms, "transforms", None) or _refuse(transforms, "the joint transform must be a Compose"))
    if not items or not isinstance(items[0], joint_transforms.RandomSizeAndCrop):
        _refuse(items[0] if items else transforms, "the joint chain starts with RandomSizeAndCrop")
    rs = items[0]
    if rs.crop_nopad or rs.pre_size is not None or rs.ignore_index != 255 or not isinstance(rs.size, int) or rs.size < 1:
        _refuse(rs, "only an integer size, crop_nopad=False, pre_size=None and ignore_index=255")
    if not 0.5 <= rs.scale_min <= rs.scale_max:
        _refuse(rs, "scales from 0.5 up (the resampling window is 9 taps at most)")
    flip, stage = False, 0
    for it in items[1:]:
        if isinstance(it, joint_transforms.Resize) and stage < 1 and it.size == (rs.size, rs.size):
            stage = 1       # never fires: the crop already has that size
        elif isinstance(it, joint_transforms.RandomHorizontallyFlip) and stage < 2:
            flip, stage = True, 2
        else:
            _refuse(it, "the joint chain is RandomSizeAndCrop [Resize(crop)] [RandomHorizontallyFlip], in that order")
    return dict(crop=rs.size, scale_min=float(rs.scale_min), scale_max=float(rs.scale_max), flip=flip, color_aug=color_aug, blur=blur), mean, std


Cityscapes_MEAN, Cityscapes_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class CityscapesDataloader(BaseDataLoader):
    """Cityscapes (fine) from <data_dir>/leftImg8bit and <data_dir>/gtFine, resident on the loader's device as bytes; every batch is a
    few launches of csrc/seg_data_ops.hip (ops.seg_crop, ops.seg_jitter, ops.seg_finish).

    The reference's arguments come first (data_loader/data_loaders.py:61-63; num_workers is accepted and ignored), then keyword-only
    device, dtype, layout and seed as the CIFAR loaders.  `transforms`, `transform` and `target_transform` are what
    `_create_transform` returns, read as a specification (read_transform_spec); transforms=None means no augmentation: full-size
    images in the files' order (validation and test).  The reference's Resize(crop) after RandomSizeAndCrop never fires -- the crop
    always has the crop size: the pad (S - h) // 2 + 1 on both sides makes the padded side at least S + 1 -- so it is accepted and
    skipped.  A batch is (data (B,3,h,w), target int64 (B,h,w)), or (names, data, target) with return_image_name.

    `__iter__` draws a whole epoch's table (seg_tables.draw_rows) from the loader's own generator with the reference's distributions:
    s ~ U(scale_min, scale_max), w, h = int(W s), int(H s), crop offsets uniform over the inclusive range, flip with p = 0.5,
    brightness / contrast / saturation ~ U(max(0, 1 - a), 1 + a), hue ~ U(-a, a), the order a uniform permutation, sigma = 0.15 +
    1.15 U.  It is not the reference's `random` / `np.random` stream (see base/base_data_loader.py): same distributions, different
    numbers.  With device "cpu" the same batches come from torch ops (seg_tables.host_*), bit for bit.  The dataset is uploaded whole;
    one that does not fit raises the allocator's error, unchanged."""

    def __init__(self, data_dir, batch_size, shuffle=True, validation_split=0.0, num_workers=0, split="train", transform=None,
                 target_transform=None, transforms=None, mode="fine", target_type="semantic", num_samples=None, return_image_name=False, *,
                 device=None, dtype=torch.float32, layout="nchw", seed=None):
        if layout not in LAYOUTS:
            raise ValueError(f"layout {layout!r}: one of {LAYOUTS}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"dtype {dtype}: float32 or bfloat16")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size {batch_size}")
        self.spec, mean, std = read_transform_spec(transforms, transform, target_transform)
        self.data_dir = data_dir
        if split == "train_val":
            dataset = ConcatArrays([CityscapesArrays(data_dir, s, mode, target_type, num_samples) for s in ("train", "val")])
        else:
            dataset = CityscapesArrays(data_dir, split, mode, target_type, num_samples)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.validation_split = validation_split
        self.shuffle = shuffle
        self.num_workers = num_workers      # accepted and ignored: nothing here runs in a worker
        self.training = self.spec is not None
        self.return_image_name = bool(return_image_name)
        self.device, self.dtype, self.layout, self.seed = torch.device(device), dtype, layout, seed
        self.H, self.W = dataset.data.shape[1:3]
        self._data = torch.from_numpy(dataset.data).to(self.device)
        self._targets = torch.from_numpy(dataset.targets).to(self.device)
        self._table = normalisation_table(mean, std, dtype).to(self.device)
        self._generator = self._seeded(seed)
        self._epoch_params = None
        self.n_samples = self._count_samples()
        self.sampler, self.valid_sampler = self._split_sampler(validation_split)

    def _count_samples(self):
        """The samples of an epoch, over which the validation split is taken: the images (a subclass may list them otherwise)."""
        return len(self.dataset)

    # ------------------------------------------------------------------ the epoch's draws
    def _draw_epoch(self):
        """int32 (n_samples, 32) header rows of one epoch (seg_tables), from the loader's generator."""
        g, n = self._generator, self.n_samples
        own = torch.arange(n) if self.sampler is None else torch.from_numpy(self.sampler.indices)
        order = own[torch.randperm(n, generator=g)] if (self.shuffle or self.sampler is not None) else own
        return self._draw_rows(order.numpy(), g)

    def _draw_rows(self, order, g):
        return seg_tables.draw_rows(order, self.W, self.H, self.spec, g)

    def batches(self, params):
        """Iterate the batches of a given table of header rows instead of a drawn one (any row count, indices may repeat): validated
        once on the host, then per batch the resampling tables are computed on the host, uploaded, and the kernels launched."""
        params = torch.as_tensor(params, dtype=torch.int32).contiguous()
        ops.check_seg_params(params, len(self._data), self.H, self.W)
        if self.spec is None and bool(((params[:, 1] != self.W) | (params[:, 2] != self.H) | (params[:, 16] != 0) | (params[:, 17] != 0)).any()):
            raise ValueError("CityscapesDataloader: a loader without transforms takes identity rows only")
        self._epoch_params = params
        return self._batches(params)

    def _batches(self, table):
        make = self._host_batch if self.device.type == "cpu" else self._device_batch
        for s in range(0, table.shape[0], self.batch_size):
            rows = table[s:s + self.batch_size]
            data, target = make(rows)
            if self.return_image_name:
                yield [self.dataset.names[i] for i in rows[:, 0].tolist()], data, target
            else:
                yield data, target

    def _new_out(self, B, h, w):
        """The (B,3,h,w)-logical tensor of the layout, uninitialised, and its buffer."""
        if self.layout == "nchw":
            buf = torch.empty((B, 3, h, w), dtype=self.dtype, device=self.device)
            return buf, buf
        ld = 3 if self.layout == "nhwc" else nn_hip._granule_up(3, self.dtype)
        buf = torch.empty((B, h, w, ld), dtype=self.dtype, device=self.device)
        return buf[..., :3].permute(0, 3, 1, 2), buf

    def _expanded(self, rows):
        S = self.spec["crop"]
        tab = seg_tables.expand(rows.numpy(), self.W, self.H, S)
        ops.check_seg_params(tab, len(self._data), self.H, self.W, S)
        return tab, S

    def _device_batch(self, rows):
        B = rows.shape[0]
        if self.spec is None:
            out, _ = self._new_out(B, self.H, self.W)
            out, target = ops.seg_finish(self._data, self._targets, rows.to(self.device), self._table, out, use_index=True, validated=True)
            return self._finish(out), target
        tab, S = self._expanded(rows)
        tab = tab.to(self.device)
        img, msk = ops.seg_crop(self._data, self._targets, tab, S, validated=True)
        if self.spec["color_aug"] > 0:
            ops.seg_jitter(img, tab, validated=True)
        out, _ = self._new_out(B, S, S)
        out, target = ops.seg_finish(img, msk, tab, self._table, out, blur=self.spec["blur"], validated=True)
        return self._finish(out), target

    def _host_batch(self, rows):
        """The same batch with torch ops on host tensors: what the kernels are a restatement of."""
        B = rows.shape[0]
        if self.spec is None:
            idx = rows[:, 0].long()
            img, msk = self._data[idx], self._targets[idx]
        else:
            tab, S = self._expanded(rows)
            img, msk = seg_tables.host_crop(self._data, self._targets, tab, S)
            if self.spec["color_aug"] > 0:
                img = seg_tables.host_jitter(img, tab)
            if self.spec["blur"]:
                img = seg_tables.host_blur(img, tab)
        out, buf = self._new_out(B, img.shape[1], img.shape[2])
        if self.layout == "padded":
            buf[..., 3:] = 0
        seg_tables.host_normalise(img, self._table, out)
        return self._finish(out), msk.long()


class CityscapesUniformDataloader(CityscapesDataloader):
    """`CityscapesDataloader` with the reference's class-uniform sampling (data_loader/data_loaders.py:83-97,
    data_loader/cityscapes.py:336-536): an epoch is a list of len(images) entries of which class_uniform_pct are crops that must
    cover the centroid of a given class in a given class_uniform_tile x class_uniform_tile tile of a given image, an equal number
    for each of the 19 classes that has a centroid at all (so the list may be shorter than the images), the rest plain images.

    The arguments are the reference's, then keyword-only device, dtype, layout and seed.  At construction one ops.seg_class_stats
    pass over the resident labels gives the centroids (uniform.class_centroids: `centroids`, per class int64 (k,3) rows
    [image, cx, cy]) and uniform.build_epoch the list (`imgs_uniform`, int64 (M,4) rows [image, has_centroid, cx, cy]), once, as
    the reference; `build_epoch()` redraws it.  class_uniform_pct == 0 runs no centroid pass and lists every image once.
    `n_samples`, `len()` and the validation split are over the list.  An epoch's table permutes the list's entries; word 0 of a
    row is the entry's image, and the crop offsets of an entry with a centroid are drawn as seg_tables.draw_rows documents, the
    reference's two quirks included.  No JSON cache is read or written: the reference's is keyed by split and tile only, so it
    is silently reused for another num_samples or data directory.  transforms=None is refused (the reference dies on an
    AttributeError); split='train_val' raises the reference's ValueError; maxSkip and coarse_boost_classes are not arguments of the
    reference's loader either."""
    num_classes = 19

    def __init__(self, data_dir, batch_size, shuffle=True, validation_split=0.0, num_workers=0, split="train", transform=None,
                 target_transform=None, transforms=None, mode="fine", target_type="semantic", class_uniform_pct=0.5, class_uniform_tile=1024,
                 num_samples=None, return_image_name=False, *, device=None, dtype=torch.float32, layout="nchw", seed=None):
        if split == "train_val":
            raise ValueError("Only support train split for Uniform Cityscapes")
        if transforms is None:
            raise ValueError("CityscapesUniformDataloader: transforms=None: the uniform loader needs the joint transform list "
                             "(RandomSizeAndCrop takes the centroid)")
        if int(class_uniform_tile) < 1:
            raise ValueError(f"CityscapesUniformDataloader: class_uniform_tile {class_uniform_tile}")
        self.class_uniform_pct, self.class_uniform_tile = class_uniform_pct, int(class_uniform_tile)
        super().__init__(data_dir, batch_size, shuffle, validation_split, num_workers, split, transform, target_transform, transforms, mode,
                         target_type, num_samples, return_image_name, device=device, dtype=dtype, layout=layout, seed=seed)

    def _count_samples(self):
        if self.class_uniform_pct > 0:
            stats = ops.seg_class_stats(self._targets, self.class_uniform_tile, self.num_classes)
            self.centroids = uniform.class_centroids(stats, self.class_uniform_tile)
        else:
            self.centroids = [np.zeros((0, 3), dtype=np.int64) for _ in range(self.num_classes)]
        return len(self.build_epoch())

    def build_epoch(self):
        """Redraw the epoch list from the loader's generator (the reference builds it once, at construction); -> imgs_uniform."""
        self.imgs_uniform = uniform.build_epoch(len(self.dataset), self.centroids, self.num_classes, self.class_uniform_pct, self._generator)
        return self.imgs_uniform

    def _draw_rows(self, order, g):
        entries = self.imgs_uniform[order]
        return seg_tables.draw_rows(entries[:, 0], self.W, self.H, self.spec, g, centroids=entries[:, 1:4])
