"""Class-uniform sampling for `CityscapesUniformDataloader`: the centroid lists and the epoch list of the reference's
data_loader/uniform.py, from the per-tile integer sums of ops.seg_class_stats instead of scipy's center_of_mass per tile and class.

A centroid is [image, cx, cy]: the tile's origin plus int(mean x), int(mean y) of the class's pixels inside the tile.  The sums are
integers (at most 2^20 per tile of 1024), so int(center_of_mass) is the floor division sum // count.  Per class the list runs over
the images in order and over an image's tiles in row-major order, as the reference's.  Nothing is cached in a file: the pass over
the resident labels costs less than reading the reference's JSON back.

The epoch list has one row [image, has_centroid, cx, cy] per sample: num_rand plain images, then num_per_class entries of every
class that has a centroid at all, each drawn as the reference draws them (a shuffled index, wrapped around), from the loader's torch
generator instead of numpy's global stream: same distribution, own stream."""
import numpy as np
import torch


def class_centroids(stats, tile):
    """[int64 (k_c, 3) rows [image, cx, cy] for c in classes] from stats (n, th, tw, C, 3) = [count, sum x, sum y]."""
    s = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    if s.ndim != 5 or s.shape[4] != 3:
        raise ValueError(f"class_centroids: stats must be (n, th, tw, C, 3), got {s.shape}")
    tile = int(tile)
    out = []
    for c in range(s.shape[3]):
        cnt = s[:, :, :, c, 0]
        img, ty, tx = np.nonzero(cnt)                   # C order: images, then an image's tiles row-major
        k = cnt[img, ty, tx]
        cx = tx * tile + s[img, ty, tx, c, 1] // k
        cy = ty * tile + s[img, ty, tx, c, 2] // k
        out.append(np.stack([img, cx, cy], axis=1).astype(np.int64).reshape(-1, 3))
    return out


def _sampling(length, num, generator):
    """`num` positions into a list of `length` items: a shuffled index, wrapped around (the reference's random_sampling)."""
    if length < 1:
        raise ValueError("build_epoch: nothing to sample from")
    perm = torch.randperm(length, generator=generator).numpy()
    return perm[np.arange(max(num, 0)) % length]


def build_epoch(n_images, centroids, num_classes, class_uniform_pct, generator):
    """int64 (M, 4) rows [image, has_centroid, cx, cy]: the reference's build_epoch.  num_per_class = int(n pct / num_classes) entries
    for every class whose list is not empty (a class with no centroid adds nothing, so M may be below n), in front of them
    n - num_classes * num_per_class plain images; pct == 0: every image once, in order."""
    n = int(n_images)
    if not class_uniform_pct > 0:
        rows = np.zeros((n, 4), dtype=np.int64)
        rows[:, 0] = np.arange(n)
        return rows
    num_per_class = int((n * class_uniform_pct) / num_classes)
    num_rand = n - num_per_class * num_classes
    plain = np.zeros((max(num_rand, 0), 4), dtype=np.int64)
    plain[:, 0] = _sampling(n, num_rand, generator)
    parts = [plain]
    for c in range(num_classes):
        lst = np.asarray(centroids[c], dtype=np.int64).reshape(-1, 3)
        if len(lst) == 0:
            continue
        pick = lst[_sampling(len(lst), num_per_class, generator)]
        part = np.ones((len(pick), 4), dtype=np.int64)
        part[:, 0], part[:, 2], part[:, 3] = pick[:, 0], pick[:, 1], pick[:, 2]
        parts.append(part)
    return np.concatenate(parts)
