"""`Cifar10Dataloader` / `Cifar100Dataloader` (reference data_loader/data_loaders.py:8-53) over base.BaseDataLoader: the dataset read
from the standard python pickles (never downloaded, no torchvision), resident on the device, one kd_cifar_batch launch per batch.

The reference's constructor arguments come first and mean what they mean there (num_workers is accepted and ignored); then,
keyword-only: device (None: the current GPU if there is one, else the CPU), dtype (float32 / bfloat16), layout ("nchw" | "nhwc" |
"padded", see BaseDataLoader) and seed.  The normalisation constants are the reference's, its quirk included: the CIFAR-10 loader
normalises with the ImageNet statistics.  The random stream is not the reference's (see base/base_data_loader.py): torchvision draws
per image from the global RNG, these loaders draw a whole epoch at a time from their own generator."""
import os
import pickle

import numpy as np
import torch

from ..base.base_data_loader import BaseDataLoader


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
