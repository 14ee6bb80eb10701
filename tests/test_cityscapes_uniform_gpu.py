"""kd_seg_class_stats and CityscapesUniformDataloader on the GPU.  The kernel sums integers, so every comparison is torch.equal
against the host path of ops.seg_class_stats (which tests/test_cityscapes_uniform_host.py holds to the reference's own centroid
lists) or against a closed form, and the kernel a call notes is the one csrc/seg_stats_select.h, compiled for the host
(tests/seg_stats_select_host), predicts for the call's pointer, width and tile.

Shapes: the 40 x 72 and 40 x 44 fixture maps at tiles 8, 16, 20 and 40 (byte loads: neither width is a multiple of 16; remainder
rows and columns at 16 and 20); seeded labels (2, 72, 160) at tiles 16, 32 and 64 (16-byte loads, remainder rows and columns, and
the same labels one byte off: byte loads); seeded labels (2, 300, 520) at tile 256 (a unit of 65536 labels: 256 loop trips a thread,
two tiles an image, remainders, 255 and an out-of-range value); one class over (1, 1024, 2048) at tile 1024 (16 units a tile) and
over (1, 4096, 4096) at tile 4096, whose column sum 4096 * 4096 * 4095 / 2 is beyond 2^32 (256 units of 16 rows)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _cityscapes_cases as K
from test_cityscapes_uniform_host import TILES, tree40, transform_args  # noqa: F401  (tree40 is a fixture)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "seg_stats_select_host")
VALUES = torch.tensor(list(range(19)) + [255, 40], dtype=torch.uint8)


def lib():
    from kdcc_amd import _lib, ops
    return _lib, ops


@pytest.fixture(scope="module")
def predicted():
    """(tensor, tile) -> the kernel name seg_stats_select.h picks for the call."""
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libseg_stats_select.so"))
    so.st_name.restype = C.c_char_p
    so.st_select.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]

    def name(t, tile):
        o = (C.c_double * 9)()
        so.st_select(t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], tile, o)
        assert int(o[1]) == 1
        return so.st_name(int(o[0])).decode()

    return name


def off_by_one(t):
    """The same labels in a tensor whose first byte sits one byte behind a 16-B boundary."""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 1
    return out


def check(host, tile, predicted, want_name, dev=None, num_classes=19):
    _lib, ops = lib()
    dev = host.cuda() if dev is None else dev
    got = ops.seg_class_stats(dev, tile, num_classes)
    name = _lib.last_plumbing_kernel()
    assert name == predicted(dev, tile) == want_name
    assert got.is_cuda and got.dtype == torch.int64
    assert torch.equal(got.cpu(), ops.seg_class_stats(host, tile, num_classes))
    return got


def seeded(shape, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return VALUES[torch.randint(0, len(VALUES), shape, generator=g)].contiguous()


@pytest.mark.parametrize("width", [72, 44])
def test_the_fixture_maps_equal_the_host_path_at_every_tile(width, predicted):
    _, masks = K.arrays(width)
    host = torch.from_numpy(np.ascontiguousarray(masks))
    dev = host.cuda()
    for tile in TILES:
        got = check(host, tile, predicted, "seg_class_stats_kernel<1>", dev)
        assert int(got[..., 0].sum()) > 0
    check(host, 16, predicted, "seg_class_stats_kernel<1>", off_by_one(dev))


@pytest.mark.parametrize("tile", [16, 32, 64])
def test_16_byte_loads_where_they_apply_and_byte_loads_one_byte_off(tile, predicted):
    host = seeded((2, 72, 160), 5)
    host[1, 8:40, 16:120] = 7                      # a run longer than a chunk: the four-compare path
    dev = host.cuda()
    assert dev.data_ptr() % 16 == 0
    a = check(host, tile, predicted, "seg_class_stats_kernel<16>", dev)
    b = check(host, tile, predicted, "seg_class_stats_kernel<1>", off_by_one(dev))
    assert torch.equal(a, b) and tuple(a.shape) == (2, 72 // tile, 160 // tile, 19, 3)
    check(host, tile, predicted, "seg_class_stats_kernel<16>", dev, num_classes=64)


def test_a_tile_of_several_loop_trips_with_remainders_and_an_out_of_range_value(predicted):
    host = seeded((2, 300, 520), 6)
    got = check(host, 256, predicted, "seg_class_stats_kernel<1>")
    assert tuple(got.shape) == (2, 1, 2, 19, 3)
    assert int(got[..., 0].sum()) == int((host[:, :256, :512] < 19).sum())
    check(host, 256, predicted, "seg_class_stats_kernel<1>", num_classes=41)


def test_two_calls_give_identical_bits(predicted):
    _, ops = lib()
    dev = seeded((2, 300, 520), 7).cuda()
    assert torch.equal(ops.seg_class_stats(dev, 256), ops.seg_class_stats(dev, 256))
    wide = seeded((3, 64, 256), 8).cuda()
    assert torch.equal(ops.seg_class_stats(wide, 64), ops.seg_class_stats(wide, 64))


@pytest.mark.parametrize("H,W,tile", [(1024, 2048, 1024), (4096, 4096, 4096)])
def test_one_class_over_a_large_tile_equals_the_closed_forms(H, W, tile, predicted):
    _lib, ops = lib()
    dev = torch.full((1, H, W), 13, dtype=torch.uint8, device="cuda")
    got = ops.seg_class_stats(dev, tile)
    assert _lib.last_plumbing_kernel() == predicted(dev, tile) == "seg_class_stats_kernel<16>"
    want = torch.zeros((1, H // tile, W // tile, 19, 3), dtype=torch.int64)
    want[..., 13, 0] = tile * tile
    want[..., 13, 1] = want[..., 13, 2] = tile * (tile * (tile - 1) // 2)
    assert tile < 4096 or int(want[0, 0, 0, 13, 1]) > 2 ** 32
    assert torch.equal(got.cpu(), want)


def test_a_tile_larger_than_the_image_gives_an_empty_result_and_no_launch():
    _lib, ops = lib()
    small = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    ops.seg_class_stats(small, 8)
    assert _lib.last_plumbing_kernel() == "seg_class_stats_kernel<1>"
    dev = torch.zeros((2, 64, 160), dtype=torch.uint8, device="cuda")
    for tile in (128, 65, 161):
        got = ops.seg_class_stats(dev, tile)
        assert got.is_cuda and tuple(got.shape) == (2, 0, 0, 19, 3)
        rc = _lib.lib().kd_seg_class_stats(C.c_void_p(dev.data_ptr()), 2, 64, 160, tile, 19, None, ops.stream_ptr())
        assert rc == 0 and _lib.last_plumbing_kernel() == "seg_class_stats_kernel<1>", "nothing was noted: nothing was launched"
    out = torch.empty((2, 1, 2, 19, 3), dtype=torch.int64, device="cuda")
    call = lambda H, W, tile, classes: _lib.lib().kd_seg_class_stats(C.c_void_p(dev.data_ptr()), 2, H, W, tile, classes,
                                                                      C.c_void_p(out.data_ptr()), ops.stream_ptr())
    assert call(64, 160, 64, 19) == 0 and _lib.last_plumbing_kernel() == "seg_class_stats_kernel<16>"
    assert call(64, 160, 64, 65) == -2 and call(64, 160, 64, 0) == -2 and call(0, 160, 64, 19) == -2 and call(64, 32769, 64, 19) == -2
    assert call(64, 160, 0, 19) == -1
    with pytest.raises(_lib.KdccError):
        _lib.check(call(64, 160, 64, 65), "kd_seg_class_stats")


@pytest.mark.parametrize("dtype,layout", [(torch.float32, "nchw"), (torch.bfloat16, "padded")])
def test_the_loader_on_the_device_equals_the_loader_on_the_host(tree40, dtype, layout):
    from kdcc_amd import data_loader
    train, _ = transform_args()
    kw = dict(class_uniform_tile=8, dtype=dtype, layout=layout, seed=4, **train)
    host = data_loader.CityscapesUniformDataloader(tree40, 4, device="cpu", **kw)
    dev = data_loader.CityscapesUniformDataloader(tree40, 4, device="cuda", **kw)
    assert all(np.array_equal(a, b) for a, b in zip(host.centroids, dev.centroids)) and sum(len(c) for c in dev.centroids) > 19
    assert np.array_equal(host.imgs_uniform, dev.imgs_uniform) and int(dev.imgs_uniform[:, 1].sum()) == 19
    hi, di = iter(host), iter(dev)
    for _ in range(2):
        (hx, ht), (dx, dt) = next(hi), next(di)
        assert dx.is_cuda and dx.dtype == dtype and tuple(dx.shape) == (4, 3, K.S, K.S)
        assert torch.equal(dx.cpu(), hx) and torch.equal(dt.cpu(), ht)
    assert torch.equal(host.epoch_params(), dev.epoch_params())
    assert sorted(dev.epoch_params()[:, 0].tolist()) == sorted(dev.imgs_uniform[:, 0].tolist()), "word 0 is the entry's image"
