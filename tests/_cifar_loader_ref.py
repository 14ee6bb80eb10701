"""Shared by tests/test_cifar_loader_host.py and tests/test_cifar_loader_gpu.py: seeded synthetic CIFAR-10 / CIFAR-100 datasets in the
on-disk python format, and the per-image oracle of the loaders' transform: pad, crop and flip with PIL -- the calls torchvision's
RandomCrop(32, padding=4) and RandomHorizontalFlip make -- then ToTensor and Normalize restated in torch."""
import os
import pickle

import numpy as np
import torch
from PIL import Image, ImageOps

C10_MEAN, C10_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)              # the reference's CIFAR-10 loader: ImageNet's
C100_MEAN, C100_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


def _rows(rng, n, classes):
    """n planar rows (R plane, G plane, B plane) and labels.  Every byte value occurs, 0 and 255 at the corners of the first images."""
    data = rng.integers(0, 256, size=(n, 3072), dtype=np.uint8)
    data[0, :256] = np.arange(256, dtype=np.uint8)
    img = data.reshape(n, 3, 32, 32)
    img[:, :, 0, 0], img[:, :, 31, 31] = 255, 0
    img[:, 0, 0, 31], img[:, 1, 31, 0] = 1, 254
    return data, [int(v) for v in rng.integers(0, classes, size=n)]


def write_cifar10(root, n_per_file, seed=0):
    """<root>/cifar-10-batches-py/{data_batch_1..5, test_batch} with n_per_file images each -> (train images (5n,32,32,3), train
    labels, test images, test labels) as the loaders must read them."""
    base = os.path.join(root, "cifar-10-batches-py")
    os.makedirs(base, exist_ok=True)
    rng = np.random.default_rng(seed)
    parts = []
    for name in [f"data_batch_{i}" for i in range(1, 6)] + ["test_batch"]:
        data, labels = _rows(rng, n_per_file, 10)
        with open(os.path.join(base, name), "wb") as f:
            pickle.dump({"data": data, "labels": labels, "batch_label": name, "filenames": [f"{name}_{i}.png" for i in range(n_per_file)]}, f)
        parts.append((data, labels))
    nhwc = lambda d: np.ascontiguousarray(d.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
    train = nhwc(np.concatenate([d for d, _ in parts[:5]])), sum((l for _, l in parts[:5]), [])
    return train[0], train[1], nhwc(parts[5][0]), parts[5][1]


def write_cifar100(root, n_train, n_test, seed=1):
    """<root>/cifar-100-python/{train, test} -> (train images, train fine labels, test images, test fine labels)."""
    base = os.path.join(root, "cifar-100-python")
    os.makedirs(base, exist_ok=True)
    rng = np.random.default_rng(seed)
    out = []
    for name, n in (("train", n_train), ("test", n_test)):
        data, fine = _rows(rng, n, 100)
        with open(os.path.join(base, name), "wb") as f:
            pickle.dump({"data": data, "fine_labels": fine, "coarse_labels": [v // 5 for v in fine], "filenames": [f"{name}_{i}.png" for i in range(n)]}, f)
        out += [np.ascontiguousarray(data.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)), fine]
    return tuple(out)


def oracle_image(img, dy, dx, flip, mean, std):
    """One (32,32,3) uint8 image -> (3,32,32) fp32: RandomCrop(32, padding=4) at offset (dy, dx), the flip, ToTensor, Normalize."""
    pil = ImageOps.expand(Image.fromarray(img), border=4, fill=0)
    pil = pil.crop((dx, dy, dx + 32, dy + 32))
    if flip:
        pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
    t = torch.from_numpy(np.array(pil, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)   # ToTensor
    m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    return t.sub_(m.view(-1, 1, 1)).div_(s.view(-1, 1, 1))                                                                       # Normalize


def oracle_batch(images, labels, params, mean, std, dtype=torch.float32):
    """params: rows [index, dy, dx, flip] -> ((B,3,32,32) dense `dtype`, (B,) int64 labels)."""
    rows = [[int(v) for v in r] for r in torch.as_tensor(params).tolist()]
    x = torch.stack([oracle_image(images[i], dy, dx, fl, mean, std) for i, dy, dx, fl in rows])
    return x.to(dtype), torch.tensor([labels[i] for i, _, _, _ in rows], dtype=torch.int64)


def extreme_params(n, count=None):
    """Every (dy, dx) in {0, 4, 8}^2 with both flip values: 18 rows, indices cycling through the dataset; repeated up to `count`
    rows (with the remaining offsets of 0..8 mixed in) when given."""
    rows = [[k % n, dy, dx, fl] for k, (dy, dx, fl) in enumerate((dy, dx, fl) for dy in (0, 4, 8) for dx in (0, 4, 8) for fl in (0, 1))]
    k = len(rows)
    while count is not None and len(rows) < count:
        rows.append([(7 * k) % n, k % 9, (k // 9) % 9, (k // 81) % 2])
        k += 1
    return torch.tensor(rows if count is None else rows[:max(count, 1)], dtype=torch.int32)


def logical(batch, dtype=None):
    """A loader's batch as a dense (B,3,32,32) tensor, whatever its layout."""
    return batch.contiguous() if dtype is None else batch.to(dtype).contiguous()
