"""Shared by tools/make_golden_hrnet.py (on the reference's HighResolutionNet) and the HRNet tests (on this package's): the narrow
config of tests/golden/hrnet.npz, the seed tag, the shipped plan shrunk to that config, and the goldens' bound rule."""
from _seeded import seeded_fill_, seeded_input  # noqa: F401
from _wrnref import project, rel_l2  # noqa: F401

TAG = "hr."
INPUT_SHAPE = (2, 3, 64, 96)          # branch maps 16x24, 8x12, 4x6, 2x3
# channels 16 / 48 / 64 / 96: both sides of the 32-channel conv granule and a padded concatenation (224 is a multiple, 16 + 48 are not)
NARROW = {
    "extra": {
        "FINAL_CONV_KERNEL": 1,
        "STAGE1": {"NUM_MODULES": 1, "NUM_RANCHES": 1, "BLOCK": "BOTTLENECK", "NUM_BLOCKS": [1], "NUM_CHANNELS": [16], "FUSE_METHOD": "SUM"},
        "STAGE2": {"NUM_MODULES": 1, "NUM_BRANCHES": 2, "BLOCK": "BASIC", "NUM_BLOCKS": [1, 1], "NUM_CHANNELS": [16, 48], "FUSE_METHOD": "SUM"},
        "STAGE3": {"NUM_MODULES": 1, "NUM_BRANCHES": 3, "BLOCK": "BASIC", "NUM_BLOCKS": [1, 1, 1], "NUM_CHANNELS": [16, 48, 64],
                   "FUSE_METHOD": "SUM"},
        "STAGE4": {"NUM_MODULES": 1, "NUM_BRANCHES": 4, "BLOCK": "BASIC", "NUM_BLOCKS": [1, 1, 1, 1], "NUM_CHANNELS": [16, 48, 64, 96],
                   "FUSE_METHOD": "SUM"},
    },
    "align_corners": True,
    "ocr.mid_channels": 64,
    "ocr.key_channels": 32,
    "num_classes": 19,
}
# the shipped plan (stage4.0.branches.3.N.conv1 / conv2, 9x9 / dilation 5 / padding 20) on the one block the narrow branch has
PLAN = ["stage4.0.branches.3.0.conv1", "stage4.0.branches.3.0.conv2"]
PLAN_ARGS = {"kernel_size": 9, "padding": 20, "dilation": 5}
HINT_CLASSES = 1000                   # hint_loss.args.num_classes of cfg/cityscapes/10M_hrnet_all.json


def bound(g, name, floor=1e-3):
    """The test bound of a stored tensor: max(the 1e-3 parity bar, 3 x the reference's own fp32-vs-fp64 rel-L2 error of it)."""
    return max(floor, 3.0 * float(g["tol:" + name]))


def seeded_target():
    """Labels for INPUT_SHAPE: classes 0..18, every 17th pixel ignored (255)."""
    import torch
    N, _, H, W = INPUT_SHAPE
    t = torch.randint(0, 19, (N, H, W), generator=torch.Generator().manual_seed(11))
    t.view(-1)[::17] = 255
    return t
