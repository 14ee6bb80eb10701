"""The rows the Cityscapes loader tests share (host and GPU): explicit draws for every resampling, jitter and blur case the kernels
can take a different path on, over the 40x72 and 40x44 fixture images with crop 24, built with the loader's own row writer."""
import itertools

import numpy as np
import torch

import _cityscapes_loader_ref as R

S = 24
SCALES = (0.5, 0.77, 1.0, 1.37, 2.0)        # 9 taps (40x44 pads both axes, 40x72 the height only), down, no pass, up, up x2
NOISE = 3                                   # the fixture's last image of each width is seeded noise
JITTER = {      # name -> (order, (brightness, contrast, saturation), hue); the others neutral where one operation stands alone
    "brightness_below": ((0, 1, 2, 3), (0.7, 1.0, 1.0), 0.0), "brightness_above": ((0, 1, 2, 3), (1.3, 1.0, 1.0), 0.0),
    "contrast_below": ((0, 1, 2, 3), (1.0, 0.7, 1.0), 0.0), "contrast_above": ((0, 1, 2, 3), (1.0, 1.3, 1.0), 0.0),
    "saturation_below": ((0, 1, 2, 3), (1.0, 1.0, 0.7), 0.0), "saturation_above": ((0, 1, 2, 3), (1.0, 1.0, 1.3), 0.0),
    "hue_negative": ((0, 1, 2, 3), (1.0, 1.0, 1.0), -0.2), "hue_positive": ((0, 1, 2, 3), (1.0, 1.0, 1.0), 0.2),
    "contrast_first": ((1, 3, 0, 2), (0.8, 1.2, 0.85), 0.13), "contrast_middle": ((2, 0, 1, 3), (1.15, 0.8, 1.2), -0.07),
    "contrast_last": ((3, 2, 0, 1), (0.9, 1.1, 1.18), 0.19),
}
HUE_CASES = tuple(k for k, v in JITTER.items() if v[2] != 0.0)
SIGMAS = (0.15, 0.6, 1.3)                   # radius 1, 2 and 5


def tables():
    from kdcc_amd.data_loader import seg_tables
    return seg_tables


def arrays(width):
    """(images (4,40,width,3), train-id masks (4,40,width)) of the fixture."""
    fx = R.fixture()
    return fx[f"img_{width}"], np.stack([R.train_ids(m) for m in fx[f"ids_{width}"]])


def resample_rows(width):
    """[(label, row)]: every scale x {offsets 0, offsets max} x {no flip, flip}, on the noise image and on a photograph."""
    T, out = tables(), []
    H, W = 40, width
    for k, (s, far, flip) in enumerate(itertools.product(SCALES, (0, 1), (0, 1))):
        w, h = int(W * s), int(H * s)
        mx, my = T.max_offsets(T.make_row(0, W, H, S, w, h, 0, 0, 0), S)
        for idx in (NOISE, k % 3):
            out.append((f"{width}-s{s}-{'max' if far else 'zero'}-{'flip' if flip else 'noflip'}-img{idx}",
                        T.make_row(idx, W, H, S, w, h, mx * far, my * far, flip)))
    return out


def plain_row(idx, width, **kw):
    """A crop at scale 1 from offset (3, 5) of image idx, with the jitter / blur draws of kw."""
    return tables().make_row(idx, width, 40, S, width, 40, 3, 5, 0, **kw)


def jitter_row(name, idx, width=72):
    order, factors, hue = JITTER[name]
    return plain_row(idx, width, order=order, factors=factors, hue=hue)


def end_to_end_rows(width):
    """Whole-chain rows: a scale and flip with a jitter order class and a blur radius each."""
    T, out = tables(), []
    H, W = 40, width
    names = ("contrast_first", "contrast_middle", "contrast_last")
    for k, (s, sigma) in enumerate(zip((0.5, 0.77, 1.0, 1.37, 2.0, 0.9), (0.15, 0.6, 1.3, 1.0, 0.3, 1.3))):
        order, factors, hue = JITTER[names[k % 3]]
        w, h = int(W * s), int(H * s)
        mx, my = T.max_offsets(T.make_row(0, W, H, S, w, h, 0, 0, 0), S)
        out.append(T.make_row((k + 3) % 4, W, H, S, w, h, mx // 2, my // 3, k % 2, order=order, factors=factors, hue=hue, sigma=sigma))
    return out


def stack(rows):
    return torch.from_numpy(np.stack(rows))
