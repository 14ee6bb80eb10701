#!/usr/bin/env python
"""Writes tests/golden/cityscapes_tiny.npz: a few 40x72 and 40x44 windows of Cityscapes sample images (image bytes and label-id
bytes only) plus one seeded noise image of each size -- flat regions hide tap errors, noise does not.

    python tools/make_golden_cityscapes.py <dir holding leftImg8bit/ and gtFine/>

Windows are cut at fixed places of the first training images in sorted order, where the label map has several classes."""
import glob
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "cityscapes_tiny.npz")
WINDOWS = ((400, 600), (520, 1200), (300, 1500))        # (top, left) in the 1024x2048 frame


def main(data):
    images = sorted(glob.glob(os.path.join(data, "leftImg8bit", "train", "*", "*_leftImg8bit.png")))[:len(WINDOWS)]
    if len(images) < len(WINDOWS):
        raise SystemExit(f"{data}: fewer than {len(WINDOWS)} training images")
    out = {}
    rng = np.random.RandomState(20240)
    for width in (72, 44):
        img, ids = [], []
        for path, (top, left) in zip(images, WINDOWS):
            lab = path.replace("leftImg8bit", "gtFine", 1).replace("_leftImg8bit.png", "_gtFine_labelIds.png")
            img.append(np.array(Image.open(path).convert("RGB"))[top:top + 40, left:left + width])
            ids.append(np.array(Image.open(lab))[top:top + 40, left:left + width].astype(np.uint8))
        img.append(rng.randint(0, 256, (40, width, 3)).astype(np.uint8))
        ids.append(rng.randint(0, 34, (40, width)).astype(np.uint8))
        out[f"img_{width}"], out[f"ids_{width}"] = np.stack(img), np.stack(ids)
    np.savez_compressed(OUT, **out)
    print(OUT, {k: v.shape for k, v in out.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
