"""`BaseDataLoader` (reference base/base_data_loader.py:7-61) for datasets of small uint8 images that live whole in device memory.

The reference's loader is a torch DataLoader over a torchvision dataset: with num_workers 0 it transforms one PIL image at a time on
the host, collates and copies the batch to the device.  Here the dataset is uploaded once, the random draws of a whole epoch are
made at `__iter__` by a host torch.Generator and uploaded as one int32 table of rows [index, dy, dx, flip], and every batch is one
kd_cifar_batch launch on the current stream (ops.cifar_batch): crop, flip, ToTensor and Normalize as a table gather.  With host
tensors (device "cpu") the same batches come from a vectorised torch composition of the same table, bit for bit.

What matches the reference: the split (`_split_sampler`: np.random.seed(0), the first len_valid shuffled indices validate, shuffle
forced off), `len()`, `drop_last=False`, the transform and its distributions (offsets uniform in 0..8, flip with p = 0.5, order a
uniform permutation), the attributes.  What does not: the random stream.  torchvision draws per image from torch's global RNG while
the batch is assembled; this loader draws per epoch from its own generator (seeded from `seed`, or from the global RNG when seed is
None, so a script's torch.manual_seed still governs).  Same distributions, different numbers."""
import numpy as np
import torch

from .. import nn_hip, ops

LAYOUTS = ("nchw", "nhwc", "padded")
PAD = 4     # RandomCrop(32, padding=4)


def normalisation_table(mean, std, dtype=torch.float32):
    """(3,256): what ToTensor then Normalize(mean, std) make of every byte value, in torchvision's order of operations; bf16 is
    rounded once, from the fp32 result."""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    t = v[None, :].repeat(3, 1).sub(m[:, None]).div(s[:, None])
    return t.to(dtype).contiguous()


class SubsetSampler:
    """The indices of one side of the validation split (the reference's SubsetRandomSampler; the loader draws the order itself)."""

    def __init__(self, indices):
        self.indices = np.asarray(indices, dtype=np.int64)

    def __len__(self):
        return len(self.indices)

    def __iter__(self):
        return iter(self.indices[torch.randperm(len(self.indices)).numpy()].tolist())


class BaseDataLoader:
    """Batches (data, target) of an image dataset with `data` (n,32,32,3) uint8 and `targets` (n), augmented when `training`.
    layout: "nchw" dense (B,3,32,32); "nhwc" the same shape channels_last-strided; "padded" a (B,3,32,32) view of a (B,32,32,G)
    buffer, G the conv K granule of the dtype, zero behind channel 3 and tagged for nn_hip's convs to read in place."""

    def __init__(self, dataset, batch_size, shuffle, validation_split, num_workers=0, *, mean, std, training=True, device=None,
                 dtype=torch.float32, layout="nchw", seed=None):
        if layout not in LAYOUTS:
            raise ValueError(f"layout {layout!r}: one of {LAYOUTS}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"dtype {dtype}: float32 or bfloat16")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size {batch_size}")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.validation_split = validation_split
        self.shuffle = shuffle
        self.num_workers = num_workers      # accepted and ignored: nothing here runs in a worker
        self.training = bool(training)
        self.device, self.dtype, self.layout, self.seed = torch.device(device), dtype, layout, seed
        self.n_samples = len(dataset)
        self.sampler, self.valid_sampler = self._split_sampler(validation_split)
        self._data = torch.as_tensor(np.ascontiguousarray(dataset.data), dtype=torch.uint8).to(self.device)
        self._labels = torch.as_tensor(np.asarray(dataset.targets), dtype=torch.int64).to(self.device)
        self._table = normalisation_table(mean, std, dtype).to(self.device)
        self._generator = self._seeded(seed)
        self._epoch_params = None

    # ------------------------------------------------------------------ the reference's split
    def _split_sampler(self, split):
        if split == 0.0:
            return None, None
        idx_full = np.arange(self.n_samples)
        np.random.seed(0)
        np.random.shuffle(idx_full)
        if isinstance(split, int):
            assert split > 0
            assert split < self.n_samples, "validation set size is configured to be larger than entire dataset."
            len_valid = split
        else:
            len_valid = int(self.n_samples * split)
        valid_idx = idx_full[0:len_valid]
        train_idx = np.delete(idx_full, np.arange(0, len_valid))
        self.shuffle = False        # mutually exclusive with a sampler, as in the reference
        self.n_samples = len(train_idx)
        return SubsetSampler(train_idx), SubsetSampler(valid_idx)

    def split_validation(self):
        """A loader over the validation indices with the same transform (augmented when training, as in the reference), sharing
        the resident dataset; None without a split."""
        if self.valid_sampler is None:
            return None
        other = object.__new__(type(self))
        other.__dict__.update(self.__dict__)
        other.sampler, other.valid_sampler = self.valid_sampler, None
        other.n_samples = len(self.valid_sampler)
        other.seed = None if self.seed is None else self.seed + 1
        other._generator = self._seeded(other.seed)
        other._epoch_params = None
        return other

    # ------------------------------------------------------------------ the epoch's draws
    @staticmethod
    def _seeded(seed):
        g = torch.Generator()
        g.manual_seed(int(torch.randint(0, 2 ** 62, ()).item()) if seed is None else int(seed))
        return g

    def __len__(self):
        return -(-self.n_samples // self.batch_size)

    def _draw_epoch(self):
        """int32 (n_samples,4) rows [index, dy, dx, flip] of one epoch, from the loader's generator."""
        g, n = self._generator, self.n_samples
        own = torch.arange(n) if self.sampler is None else torch.from_numpy(self.sampler.indices)
        order = own[torch.randperm(n, generator=g)] if (self.shuffle or self.sampler is not None) else own
        p = torch.empty((n, 4), dtype=torch.int32)
        p[:, 0] = order
        if self.training:
            p[:, 1:3] = torch.randint(0, 2 * PAD + 1, (n, 2), generator=g)
            p[:, 3] = torch.randint(0, 2, (n,), generator=g)
        else:
            p[:, 1:3], p[:, 3] = PAD, 0
        return p

    def epoch_params(self):
        """The table of the epoch most recently started (host int32 (m,4)), None before the first."""
        return self._epoch_params

    def __iter__(self):
        return self.batches(self._draw_epoch())

    def batches(self, params):
        """Iterate the batches of a given table of rows [index, dy, dx, flip] instead of a drawn one (any row count, indices may
        repeat): validated once, uploaded in one copy, then one launch per batch."""
        params = torch.as_tensor(params, dtype=torch.int32).contiguous()
        ops.check_cifar_params(params, len(self._labels))
        self._epoch_params = params
        return self._batches(params.to(self.device))

    def _batches(self, table):
        make = self._host_batch if self.device.type == "cpu" else self._device_batch
        for s in range(0, table.shape[0], self.batch_size):
            yield make(table[s:s + self.batch_size])

    def _new_out(self, B):
        """The (B,3,32,32)-logical tensor of the layout, uninitialised, and its buffer."""
        if self.layout == "nchw":
            buf = torch.empty((B, 3, 32, 32), dtype=self.dtype, device=self.device)
            return buf, buf
        ld = 3 if self.layout == "nhwc" else nn_hip._granule_up(3, self.dtype)
        buf = torch.empty((B, 32, 32, ld), dtype=self.dtype, device=self.device)
        return buf[..., :3].permute(0, 3, 1, 2), buf

    def _finish(self, out):
        return nn_hip.mark_padded(out) if self.layout == "padded" else out

    def _device_batch(self, rows):
        out, _ = self._new_out(rows.shape[0])
        out, target = ops.cifar_batch(self._data, self._labels, rows, self._table, out, validated=True)
        return self._finish(out), target

    def _host_batch(self, rows):
        """The same batch with torch ops on host tensors: what the kernel is a restatement of."""
        rows = rows.long()
        idx, dy, dx, flip = rows.unbind(1)
        B = rows.shape[0]
        padded = torch.nn.functional.pad(self._data[idx], (0, 0, PAD, PAD, PAD, PAD))      # (B,40,40,3), zeros around: PIL's fill=0
        ar = torch.arange(32)
        ys = dy[:, None] + ar[None, :]
        xs = dx[:, None] + torch.where(flip[:, None] != 0, 31 - ar[None, :], ar[None, :])
        crop = padded[torch.arange(B)[:, None, None], ys[:, :, None], xs[:, None, :]]       # (B,32,32,3) bytes
        val = self._table.t()[crop.long(), torch.arange(3)]                                 # table[c][byte], (B,32,32,3)
        out, buf = self._new_out(B)
        if self.layout == "padded":
            buf[..., 3:] = 0
        out.copy_(val.permute(0, 3, 1, 2))
        return self._finish(out), self._labels[idx]
