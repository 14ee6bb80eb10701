"""`CityscapesArrays`: the fine Cityscapes split of the reference's data_loader/cityscapes.py:15-225, decoded once into bytes.

leftImg8bit/<split>/<city>/*_leftImg8bit.png and gtFine/<split>/<city>/*_gtFine_labelIds.png are listed in sorted order (so every
process lists the same ranks), decoded with PIL on a thread pool, the label ids remapped to train ids once; `data` (n,H,W,3) and
`targets` (n,H,W) are uint8.  Nothing is extracted from an archive or downloaded."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

IGNORE = 255
ID_TO_TRAINID = {-1: IGNORE, 0: IGNORE, 1: IGNORE, 2: IGNORE, 3: IGNORE, 4: IGNORE, 5: IGNORE, 6: IGNORE, 7: 0, 8: 1, 9: IGNORE,
                 10: IGNORE, 11: 2, 12: 3, 13: 4, 14: IGNORE, 15: IGNORE, 16: IGNORE, 17: 5, 18: IGNORE, 19: 6, 20: 7, 21: 8, 22: 9,
                 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 29: IGNORE, 30: IGNORE, 31: 16, 32: 17, 33: 18}


def _lut():
    lut = np.arange(256, dtype=np.uint8)        # ids the mapping does not name stay as they are, as in the reference
    for k, v in ID_TO_TRAINID.items():
        if k >= 0:
            lut[k] = v
    return lut


class CityscapesArrays:
    ignore_label = IGNORE

    def __init__(self, root, split="train", mode="fine", target_type="semantic", num_samples=None):
        if mode == "coarse":
            raise NotImplementedError("CityscapesArrays: mode='coarse' (gtCoarse) is not implemented, only the fine split")
        if mode != "fine":
            raise ValueError(f"CityscapesArrays: mode {mode!r}: 'fine'")
        if target_type != "semantic" and target_type != ["semantic"]:
            raise NotImplementedError(f"CityscapesArrays: target_type {target_type!r} is not implemented, only 'semantic'")
        if split not in ("train", "val", "test"):
            raise ValueError(f"CityscapesArrays: split {split!r}: one of 'train', 'val', 'test'")
        self.root, self.split, self.mode, self.target_type = root, split, "gtFine", [target_type] if isinstance(target_type, str) else target_type
        self.id_to_trainid = dict(ID_TO_TRAINID)
        self.images_dir = os.path.join(root, "leftImg8bit", split)
        self.targets_dir = os.path.join(root, "gtFine", split)
        for d in (self.images_dir, self.targets_dir):
            if not os.path.isdir(d):
                raise FileNotFoundError(f"{d}: no such directory (the dataset is read from disk, never extracted or downloaded)")
        images, targets = [], []
        for city in sorted(os.listdir(self.images_dir)):
            img_dir = os.path.join(self.images_dir, city)
            if not os.path.isdir(img_dir):
                continue
            for name in sorted(os.listdir(img_dir)):
                if not name.endswith(".png"):
                    continue
                images.append(os.path.join(img_dir, name))
                targets.append(os.path.join(self.targets_dir, city, name.split("_leftImg8bit")[0] + "_gtFine_labelIds.png"))
        if not images:
            raise FileNotFoundError(f"{self.images_dir}: no <city>/*.png images")
        for path in targets:
            if not os.path.isfile(path):
                raise FileNotFoundError(f"{path}: missing label file")
        if num_samples is not None and num_samples < len(images):
            idx = np.random.choice(len(images), num_samples)        # with replacement, from numpy's global stream, as the reference
            images, targets = [images[i] for i in idx], [targets[i] for i in idx]
        self.images, self.label_files = images, targets
        self.names = [os.path.splitext(os.path.basename(p))[0] for p in images]
        self._decode()

    def _decode(self):
        from PIL import Image
        lut = _lut()

        def one(i):
            with Image.open(self.images[i]) as im:
                a = np.asarray(im.convert("RGB"))
            with Image.open(self.label_files[i]) as im:
                t = np.asarray(im)
            if t.ndim != 2 or t.shape != a.shape[:2]:
                raise ValueError(f"{self.label_files[i]}: a label map of shape {t.shape} for an image of {a.shape[:2]}")
            return a, lut[t.astype(np.uint8)]

        first, first_t = one(0)
        H, W = first.shape[:2]
        n = len(self.images)
        self.data = np.empty((n, H, W, 3), dtype=np.uint8)
        self.targets = np.empty((n, H, W), dtype=np.uint8)

        def fill(i):
            a, t = (first, first_t) if i == 0 else one(i)
            if a.shape[:2] != (H, W):
                raise ValueError(f"{self.images[i]}: {a.shape[1]}x{a.shape[0]} pixels where {self.images[0]} has {W}x{H}: images of "
                                 "differing size cannot share the resident array")
            self.data[i], self.targets[i] = a, t

        with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as pool:
            list(pool.map(fill, range(n)))

    def __len__(self):
        return len(self.data)


class ConcatArrays:
    """split='train_val': the training images followed by the validation images, as the reference's ConcatDataset."""

    def __init__(self, parts):
        shapes = {p.data.shape[1:] for p in parts}
        if len(shapes) != 1:
            raise ValueError(f"train and val images of differing size {sorted(shapes)} cannot share the resident array")
        self.datasets = list(parts)
        self.data = np.concatenate([p.data for p in parts])
        self.targets = np.concatenate([p.targets for p in parts])
        self.names = [n for p in parts for n in p.names]
        self.images = [n for p in parts for n in p.images]
        self.id_to_trainid = parts[0].id_to_trainid
        self.ignore_label = IGNORE

    def __len__(self):
        return len(self.data)
