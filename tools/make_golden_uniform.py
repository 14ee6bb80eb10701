#!/usr/bin/env python3
"""Generate tests/golden/cityscapes_uniform.npz by running the REFERENCE's class-uniform sampling code itself (CPU): integers and the
scripted draws that produced them, nothing else.  The reference's data_loader/uniform.py and data_loader/joint_transforms.py are
imported at run time from the directory $KD_REFERENCE names; no reference source is copied.

    KD_REFERENCE=<the reference checkout> python3 tools/make_golden_uniform.py

cen_<width>_<tree>_t<tile>  int64 (k,4) rows [class, image, cx, cy]: uniform.class_centroids_all over the fixture label maps of
    tests/golden/cityscapes_tiny.npz written as PNGs to a temporary tree, per class in the reference's list order.  <tree> is `all`
    (images 0-3; the noise image 3 holds all 19 classes) or `first3` (images 0-2: some classes have no centroid).
crop_int  int64 (m,6) rows [width, S, cx, cy, x1, y1] and crop_f float64 (m,3) rows [scale, ux, uy]: the box RandomSizeAndCrop(S,
    False, scale_min=scale, scale_max=scale, ignore_index=255) crops from a 40 x width image for the centroid (cx, cy) when
    `random` is a scripted stand-in whose randint(a, b) answers a + min(int(u * (b - a + 1)), b - a), u = ux for the first call
    and uy for the second.  The box is what the reference hands to PIL's Image.crop, recorded there."""
import importlib.util
import itertools
import os
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("KD_REFERENCE") or sys.exit("set KD_REFERENCE to the reference checkout")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cityscapes_loader_ref as R                                         # noqa: E402

TILES = (8, 16, 20, 40)
S, H = 24, 40
TOP = 1.0 - 2.0 ** -53          # the largest double below 1: the upper end of randint's range


def ref_module(name):
    spec = importlib.util.spec_from_file_location("kd_reference_" + name, os.path.join(REF, "data_loader", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def centroid_lists(uniform, ids, tile):
    with tempfile.TemporaryDirectory() as root:
        names = R.write_tree(root, "train", np.zeros(ids.shape + (3,), dtype=np.uint8), ids)
        items = [(os.path.join(root, "leftImg8bit", "train", "tinytown", n + ".png"),
                  os.path.join(root, "gtFine", "train", "tinytown", n.replace("_leftImg8bit", "_gtFine_labelIds") + ".png")) for n in names]
        index = {it[0]: i for i, it in enumerate(items)}
        cen = uniform.class_centroids_all(items, 19, id2trainid=R.ID_TO_TRAINID, tile_size=tile)
    rows = [(c, index[img], xy[0], xy[1]) for c in range(19) for img, _, xy, cls in cen.get(c, []) if cls == c]
    assert len(rows) == sum(len(v) for v in cen.values())
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)


class Scripted:
    """`random` for one call of RandomSizeAndCrop: uniform answers the scale, the two randint calls the scripted positions."""

    def __init__(self, us):
        self.us = list(us)

    def uniform(self, a, b):
        assert a == b
        return a

    def randint(self, a, b):
        u = self.us.pop(0)
        return a + min(int(u * (b - a + 1)), b - a)


def crop_boxes(jt):
    ints, floats = [], []
    boxes = []
    crop = Image.Image.crop

    def recording(self, box=None):
        boxes.append(tuple(box))
        return crop(self, box)

    for width, scale in itertools.product((72, 44), (0.5, 1.0, 2.0)):
        cents = ((0, 0), (width - 1, H - 1), (width // 3, H // 2))
        draws = ((0.0, 0.0), (TOP, TOP), (0.37, 0.81))
        for (cx, cy), (ux, uy) in itertools.product(cents, draws):
            jt.random = Scripted((ux, uy))
            op = jt.RandomSizeAndCrop(S, False, scale_min=scale, scale_max=scale, ignore_index=255)
            img, mask = Image.new("RGB", (width, H)), Image.new("L", (width, H))
            del boxes[:]
            Image.Image.crop = recording
            try:
                ci, cm = op(img, mask, (cx, cy))
            finally:
                Image.Image.crop = crop
            assert ci.size == (S, S) and cm.size == (S, S) and len(boxes) == 2 and boxes[0] == boxes[1] and not jt.random.us
            x1, y1, x2, y2 = boxes[0]
            assert (x2 - x1, y2 - y1) == (S, S)
            ints.append((width, S, cx, cy, x1, y1))
            floats.append((scale, ux, uy))
    return np.asarray(ints, dtype=np.int64), np.asarray(floats, dtype=np.float64)


def main():
    uniform, jt = ref_module("uniform"), ref_module("joint_transforms")
    fx = R.fixture()
    out = {}
    for width in (72, 44):
        ids = fx[f"ids_{width}"]
        for tree, part in (("all", ids), ("first3", ids[:3])):
            for tile in TILES:
                out[f"cen_{width}_{tree}_t{tile}"] = centroid_lists(uniform, part, tile)
    out["crop_int"], out["crop_f"] = crop_boxes(jt)
    path = os.path.join(ROOT, "tests", "golden", "cityscapes_uniform.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {sum(len(v) for k, v in out.items() if k.startswith('cen_'))} centroids, "
          f"{len(out['crop_int'])} crop boxes")


if __name__ == "__main__":
    main()
