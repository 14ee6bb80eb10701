"""kdcc_amd.data_loader.CityscapesUniformDataloader without a GPU: the host path of ops.seg_class_stats and uniform.class_centroids
against the centroid lists the reference's own data_loader/uniform.py produced (tests/golden/cityscapes_uniform.npz, written by
tools/make_golden_uniform.py), build_epoch's counts and wrap-around rule, the centroid-aware crop offsets of seg_tables.draw_rows
against the boxes the reference's RandomSizeAndCrop cropped for scripted draws, the loader on throw-away trees of tiny PNGs and from
the two shipped analysis configs, its refusals, and csrc/seg_stats_select.h compiled for the host (tests/seg_stats_select_host) held
to a restated selection on both sides of every gate.

Everything here is integers, so every comparison is equality."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _cityscapes_cases as K
import _cityscapes_loader_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "seg_stats_select_host")
CSRC = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
TILES = (8, 16, 20, 40)
S = K.S


def DL():
    from kdcc_amd import data_loader
    return data_loader


def U():
    from kdcc_amd.data_loader import uniform
    return uniform


def ops():
    from kdcc_amd import ops
    return ops


def transform_args(crop=S, color_aug=0.2, blur="gaussian", scale_min=0.5, scale_max=2.0):
    cfg = {"transforms": {"joint_transforms": {"crop_size": crop, "scale_min": scale_min, "scale_max": scale_max, "ignore_label": 255},
                          "extended_transforms": {"color_aug": color_aug, "blur": blur}}}
    joint, image, target, val = DL()._create_transform(cfg)
    return dict(transforms=joint, transform=image, target_transform=target), dict(transform=val, target_transform=target)


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def golden_lists(golden, width, tree, tile):
    """[(k,3) rows [image, cx, cy] per class] of the reference."""
    rows = golden("cityscapes_uniform")[f"cen_{width}_{tree}_t{tile}"]
    return [rows[rows[:, 0] == c][:, 1:] for c in range(19)]


def write_repeated(root, width, images, times):
    """`times` copies of the fixture images `images` of one width, numbered on: -> the number of files."""
    fx = R.fixture()
    img, ids = fx[f"img_{width}"][list(images)], fx[f"ids_{width}"][list(images)]
    for k in range(times):
        R.write_tree(root, "train", img, ids, start=k * len(images))
    return times * len(images)


@pytest.fixture(scope="module")
def tree40(tmp_path_factory):
    """40 files: the four 40x72 fixture images ten times over; file i is image i % 4."""
    root = str(tmp_path_factory.mktemp("uniform40"))
    assert write_repeated(root, 72, range(4), 10) == 40
    return root


@pytest.fixture(scope="module")
def tree30(tmp_path_factory):
    """30 files of images 0-2 only: classes without a centroid."""
    root = str(tmp_path_factory.mktemp("uniform30"))
    assert write_repeated(root, 72, range(3), 10) == 30
    return root


# ------------------------------------------------------------------------------------------------ the centroids
@pytest.mark.parametrize("width", [72, 44])
@pytest.mark.parametrize("tile", TILES)
def test_host_stats_and_centroids_equal_the_references_lists(golden, width, tile):
    _, masks = K.arrays(width)
    for tree, part in (("all", masks), ("first3", masks[:3])):
        t = torch.from_numpy(np.ascontiguousarray(part))
        stats = ops().seg_class_stats(t, tile)
        assert stats.dtype == torch.int64 and tuple(stats.shape) == (len(part), 40 // tile, width // tile, 19, 3)
        got, want = U().class_centroids(stats, tile), golden_lists(golden, width, tree, tile)
        assert len(got) == 19
        for c in range(19):
            assert got[c].dtype == np.int64 and np.array_equal(got[c], want[c]), f"{tree}: class {c}"
    assert sum(len(g) for g in got) > 0 and any(len(g) == 0 for g in got), "images 0-2 lack some classes"


def test_remainder_rows_and_columns_belong_to_no_tile_and_a_large_tile_gives_no_tiles():
    _, m72 = K.arrays(72)
    _, m44 = K.arrays(44)
    t72, t44 = torch.from_numpy(m72), torch.from_numpy(m44)
    s = ops().seg_class_stats(t72, 16)
    assert tuple(s.shape[1:3]) == (2, 4), "40 x 72 at tile 16: 8 remainder rows and 8 remainder columns"
    assert int(s[..., 0].sum()) == int((t72[:, :32, :64] < 19).sum()) < int((t72 < 19).sum())
    assert torch.equal(s, ops().seg_class_stats(t72[:, :32, :64].contiguous(), 16))
    s = ops().seg_class_stats(t44, 20)
    assert tuple(s.shape[1:3]) == (2, 2) and torch.equal(s, ops().seg_class_stats(t44[:, :, :40].contiguous(), 20)), "4 remainder columns"
    for t in (t72, t44):
        s = ops().seg_class_stats(t, 64)
        assert s.numel() == 0 and tuple(s.shape) == (4, 0, 0, 19, 3)
        assert all(len(c) == 0 and c.shape == (0, 3) for c in U().class_centroids(s, 64))


def test_ignored_and_out_of_range_labels_count_nowhere_and_the_sums_are_the_closed_forms():
    t = torch.full((1, 8, 12), 255, dtype=torch.uint8)
    t[0, 1, 2] = 5
    t[0, 3, 7] = 5
    t[0, 2, 2] = 40
    t[0, 0, 0] = 19
    s = ops().seg_class_stats(t, 4)
    assert int(s.sum()) == int(s[0, :, :, 5].sum()) and s[0, 0, 0, 5].tolist() == [1, 2, 1] and s[0, 0, 1, 5].tolist() == [1, 3, 3]
    assert ops().seg_class_stats(t, 4, num_classes=41)[0, 0, 0, 40].tolist() == [1, 2, 2]
    full = torch.full((2, 6, 6), 3, dtype=torch.uint8)
    assert ops().seg_class_stats(full, 6, 4)[:, 0, 0, 3].tolist() == [[36, 6 * 15, 6 * 15]] * 2
    with pytest.raises(ValueError):
        ops().seg_class_stats(t, 0)
    with pytest.raises(ValueError):
        ops().seg_class_stats(t, 4, num_classes=65)
    with pytest.raises(ValueError):
        ops().seg_class_stats(t.long(), 4)


# ------------------------------------------------------------------------------------------------ the epoch list
def centroids_of(width, images, times, tile):
    _, masks = K.arrays(width)
    t = torch.from_numpy(np.ascontiguousarray(np.concatenate([masks[list(images)]] * times)))
    return U().class_centroids(ops().seg_class_stats(t, tile), tile)


def test_build_epoch_on_40_files_is_21_plain_images_and_one_entry_per_class():
    cen = centroids_of(72, range(4), 10, 40)
    assert all(len(c) >= 10 for c in cen), "the noise image, ten times over, holds every class"
    ep = U().build_epoch(40, cen, 19, 0.5, gen(3))
    assert ep.dtype == np.int64 and ep.shape == (21 + 19, 4), "int(40 * 0.5 / 19) = 1 per class, 40 - 19 plain"
    plain, uni = ep[:21], ep[21:]
    assert np.all(plain[:, 1:] == 0) and len(set(plain[:, 0].tolist())) == 21 and plain[:, 0].min() >= 0 and plain[:, 0].max() < 40
    assert np.all(uni[:, 1] == 1)
    for c in range(19):
        assert any(np.array_equal(uni[c, [0, 2, 3]], row) for row in cen[c]), f"the entry of class {c} is one of its centroids"
    again = U().build_epoch(40, cen, 19, 0.5, gen(3))
    assert np.array_equal(ep, again) and not np.array_equal(ep, U().build_epoch(40, cen, 19, 0.5, gen(4)))


def test_build_epoch_skips_classes_without_a_centroid():
    cen = centroids_of(72, range(3), 10, 40)
    empty = [c for c in range(19) if len(cen[c]) == 0]
    assert 0 < len(empty) < 19
    ep = U().build_epoch(30, cen, 19, 0.7, gen(5))
    per = int(30 * 0.7 / 19)
    assert per == 1 and ep.shape == (30 - 19 * per + (19 - len(empty)) * per, 4) and len(ep) < 30
    uni = ep[30 - 19 * per:]
    present = [c for c in range(19) if len(cen[c])]
    for k, c in enumerate(present):
        assert any(np.array_equal(uni[k, [0, 2, 3]], row) for row in cen[c])


def test_build_epoch_wraps_around_a_short_list():
    cen = [np.zeros((0, 3), dtype=np.int64) for _ in range(19)]
    cen[4] = np.array([[0, 1, 2], [1, 3, 4], [2, 5, 6]])
    cen[7] = np.array([[3, 7, 8]])
    ep = U().build_epoch(190, cen, 19, 0.85, gen(9))
    per = int(190 * 0.85 / 19)
    assert per == 8 and ep.shape == (190 - 19 * 8 + 2 * 8, 4)
    uni = ep[190 - 19 * 8:]
    counts = [int((uni[:8, [0, 2, 3]] == row).all(1).sum()) for row in cen[4]]
    assert sorted(counts) == [2, 3, 3] and sum(counts) == 8, "8 draws from 3 centroids: floor or ceil of 8 / 3 each"
    assert np.all(uni[8:, [0, 2, 3]] == cen[7][0]) and np.all(uni[:, 1] == 1)
    plain = ep[:38, 0]
    assert len(set(plain.tolist())) == 38
    many = U().build_epoch(5, cen, 19, 0.0, gen(9))
    assert np.array_equal(many, np.stack([np.arange(5), np.zeros(5), np.zeros(5), np.zeros(5)], 1).astype(np.int64)), "pct 0: the identity list"


# ------------------------------------------------------------------------------------------------ the crop offsets
def scripted(monkeypatch, u):
    """torch.rand answers the (n,9) uniforms u while the context lasts."""
    u = torch.as_tensor(np.asarray(u, dtype=np.float64))

    def rand(shape, generator=None, dtype=None):
        assert tuple(shape) == tuple(u.shape) and dtype == torch.float64
        return u.clone()

    monkeypatch.setattr(torch, "rand", rand)


def test_draw_rows_reproduces_the_references_boxes_for_its_scripted_draws(golden, monkeypatch):
    T = K.tables()
    z = golden("cityscapes_uniform")
    ints, floats = z["crop_int"], z["crop_f"]
    assert len(ints) == 54 and set(ints[:, 0]) == {72, 44} and set(floats[:, 0]) == {0.5, 1.0, 2.0}
    clamped_low = clamped_high = padded = 0
    for (width, crop, cx, cy, x1, y1), (scale, ux, uy) in zip(ints.tolist(), floats.tolist()):
        spec = dict(crop=int(crop), scale_min=scale, scale_max=scale, flip=False, color_aug=0.0, blur=False)
        u = np.zeros((1, 9))
        u[0, 1], u[0, 2] = ux, uy
        scripted(monkeypatch, u)
        row = T.draw_rows(np.array([2]), int(width), 40, spec, None, centroids=np.array([[1, cx, cy]])).numpy()[0]
        assert (row[0], row[1], row[2]) == (2, int(width * scale), int(40 * scale))
        assert (row[5], row[6]) == (x1, y1), f"width {width} scale {scale} centroid ({cx}, {cy}) u ({ux}, {uy})"
        plain = T.draw_rows(np.array([2]), int(width), 40, spec, None, centroids=np.array([[0, cx, cy]])).numpy()[0]
        mx, my = T.max_offsets(row, int(crop))
        assert (plain[5], plain[6]) == (min(int(ux * (mx + 1)), mx), min(int(uy * (my + 1)), my)), "has_centroid 0: cropped as today"
        clamped_low += int(x1 == 0 and int(cx * scale) - crop + int(ux * (crop + 1)) < 0)
        clamped_high += int(x1 == mx and min(int(cx * scale) - crop + int(ux * (crop + 1)), int(cx * scale)) > mx)
        padded += int(row[3] > 0 and row[4] > 0)
    assert clamped_low and clamped_high and padded, "both clamps and the padded case S > h, S > w occur"


def test_draw_rows_without_centroids_draws_exactly_the_rows_it_drew_before_the_argument_existed():
    T = K.tables()
    spec = dict(crop=24, scale_min=0.5, scale_max=2.0, flip=True, color_aug=0.2, blur=True)
    order = np.arange(50) % 4
    before = T.draw_rows(order, 72, 40, spec, gen(17)).numpy()                     # positionally, as the plain loader calls it
    g = gen(17)
    assert np.array_equal(T.draw_rows(order, 72, 40, spec, g, None).numpy(), before)
    state = g.get_state()
    none = np.zeros((50, 3), dtype=np.int64)
    g2 = gen(17)
    assert np.array_equal(T.draw_rows(order, 72, 40, spec, g2, centroids=none).numpy(), before), "has_centroid 0 everywhere"
    assert torch.equal(g2.get_state(), state), "the same uniforms are consumed"
    cen = np.stack([np.ones(50), np.full(50, 71), np.full(50, 39)], 1).astype(np.int64)
    g3 = gen(17)
    with_c = T.draw_rows(order, 72, 40, spec, g3, centroids=cen).numpy()
    assert torch.equal(g3.get_state(), state)
    other = [c for c in range(32) if c not in (5, 6)]
    assert np.array_equal(with_c[:, other], before[:, other]) and not np.array_equal(with_c[:, 5:7], before[:, 5:7])
    # the pinned words of the first row of this seed: a change of the stream shows here
    assert before.shape == (50, 32) and np.array_equal(before[:, 0], order)
    assert np.array_equal(T.draw_rows(order, 72, 40, None, gen(17), centroids=cen).numpy(), np.stack([T.identity_row(i, 72, 40) for i in order]))


# ------------------------------------------------------------------------------------------------ the loader
def test_the_loader_on_the_40_file_tree(tree40):
    train, _ = transform_args()
    L = DL().CityscapesUniformDataloader(tree40, 4, class_uniform_tile=40, device="cpu", seed=2, **train)
    assert isinstance(L, DL().CityscapesDataloader) and len(L.dataset) == 40
    assert len(L.centroids) == 19 and all(c.shape[1] == 3 and len(c) >= 10 for c in L.centroids)
    assert L.imgs_uniform.shape == (40, 4) and L.n_samples == 40 and len(L) == 10
    assert int(L.imgs_uniform[:, 1].sum()) == 19
    first = L.imgs_uniform.copy()
    batches = list(L)
    assert len(batches) == 10 and all(x.shape == (4, 3, S, S) and t.shape == (4, S, S) and t.dtype == torch.int64 for x, t in batches)
    p = L.epoch_params()
    assert p.shape == (40, 32) and sorted(p[:, 0].tolist()) == sorted(first[:, 0].tolist()), "an epoch's table permutes the list's entries"
    again = list(L.batches(p))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(batches, again))
    assert np.array_equal(L.imgs_uniform, first), "the list is built once, not per epoch"
    assert L.build_epoch() is L.imgs_uniform and L.imgs_uniform.shape == (40, 4) and not np.array_equal(L.imgs_uniform, first)
    same = DL().CityscapesUniformDataloader(tree40, 4, class_uniform_tile=40, device="cpu", seed=2, **train)
    assert np.array_equal(same.imgs_uniform, first) and torch.equal(next(iter(same))[0], batches[0][0])
    assert not [f for f in os.listdir(os.getcwd()) if f.startswith("cityscapes_") and f.endswith(".json")], "no JSON cache"


def test_the_loader_lists_fewer_samples_when_classes_lack_centroids_and_splits_over_the_list(tree30):
    train, _ = transform_args()
    L = DL().CityscapesUniformDataloader(tree30, 4, validation_split=0.25, class_uniform_pct=0.7, class_uniform_tile=40, device="cpu", seed=1, **train)
    empty = sum(len(c) == 0 for c in L.centroids)
    M = 30 - empty
    assert 0 < empty < 19 and len(L.imgs_uniform) == M and len(L.dataset) == 30
    n_valid = int(M * 0.25)
    assert L.n_samples == M - n_valid and len(L) == -(-(M - n_valid) // 4)
    valid = L.split_validation()
    assert valid.n_samples == n_valid and sorted(L.sampler.indices.tolist() + valid.sampler.indices.tolist()) == list(range(M))
    list(valid)
    assert sorted(valid.epoch_params()[:, 0].tolist()) == sorted(L.imgs_uniform[valid.sampler.indices, 0].tolist())


def test_pct_zero_runs_no_centroid_pass_and_lists_every_image(tree30, monkeypatch):
    train, _ = transform_args()

    def never(*a, **k):
        raise AssertionError("class_uniform_pct == 0 runs no centroid pass")

    monkeypatch.setattr(ops(), "seg_class_stats", never)
    L = DL().CityscapesUniformDataloader(tree30, 7, class_uniform_pct=0, device="cpu", seed=1, return_image_name=True, **train)
    assert np.array_equal(L.imgs_uniform[:, 0], np.arange(30)) and not L.imgs_uniform[:, 1:].any() and all(len(c) == 0 for c in L.centroids)
    names, x, t = next(iter(L))
    assert names == [L.dataset.names[i] for i in L.epoch_params()[:7, 0].tolist()] and x.shape == (7, 3, S, S)


@pytest.mark.parametrize("name", ["deeplabwv3p", "gscnn"])
def test_the_analysis_configs_construct_their_training_loader_unchanged(tree40, tmp_path, name):
    import kdcc_amd
    from kdcc_amd import ConfigParser
    with open(os.path.join(HERE, "golden", "cfg", "cityscapes", "analysis_compressible", name + ".json")) as f:
        cfg = json.load(f)
    block = cfg["train_data_loader"]
    assert block["type"] == "CityscapesUniformDataloader"
    block["args"]["data_dir"] = tree40
    if "save_dir" in cfg.get("trainer", {}):
        cfg["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfg, run_id=name)
    joint, image, target, _ = kdcc_amd.data_loader._create_transform(config)
    L = config.init_obj("train_data_loader", kdcc_amd.data_loader, transforms=joint, transform=image, target_transform=target,
                        device="cpu", seed=0)
    assert type(L).__name__ == "CityscapesUniformDataloader" and L.class_uniform_tile == 1024 and L.class_uniform_pct == 0.5
    assert L.imgs_uniform.shape == (40 - 19, 4) and not L.imgs_uniform[:, 1].any(), "tile 1024 on 40 x 72 maps: no tile, no centroid"
    crop = cfg["transforms"]["joint_transforms"]["crop_size"]
    x, t = next(iter(L))
    assert tuple(x.shape) == (block["args"]["batch_size"], 3, crop, crop) and tuple(t.shape) == (block["args"]["batch_size"], crop, crop)


def test_the_three_refusals(tree40):
    train, val = transform_args()
    L = DL().CityscapesUniformDataloader
    with pytest.raises(ValueError, match="joint transform list"):
        L(tree40, 1, device="cpu", **val)
    with pytest.raises(ValueError, match="^Only support train split for Uniform Cityscapes$"):
        L(tree40, 1, split="train_val", device="cpu", **train)
    with pytest.raises(NotImplementedError, match="coarse"):
        L(tree40, 1, mode="coarse", device="cpu", **train)
    import inspect
    params = list(inspect.signature(L.__init__).parameters)
    assert params[1:17] == ["data_dir", "batch_size", "shuffle", "validation_split", "num_workers", "split", "transform", "target_transform",
                            "transforms", "mode", "target_type", "class_uniform_pct", "class_uniform_tile", "num_samples", "return_image_name",
                            "device"]
    assert "maxSkip" not in params and "coarse_boost_classes" not in params
    with pytest.raises(FileNotFoundError):
        L(tree40, 1, split="val", device="cpu", **train)       # every other split is accepted: this tree has no val folder


# ------------------------------------------------------------------------------------------------ seg_stats_select.h
FIELDS = ("kernel", "launch", "vec", "th", "tw", "rows", "chunks", "units", "grid")
CONSTS = ("TPB", "MAX_CLASSES", "WG_BYTES", "MAX_GRID", "MAX_SIDE", "SSK_STATS_1", "SSK_STATS_16")
BASE = 0x10000


@pytest.fixture(scope="module")
def sel():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libseg_stats_select.so"))
    so.st_name.restype = C.c_char_p
    so.st_const.restype = C.c_longlong
    so.st_rows.argtypes = [C.c_int, C.c_longlong]
    so.st_select.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    return so


def select(so, n, H, W, tile, off=0):
    o = (C.c_double * len(FIELDS))()
    so.st_select(BASE + off, n, H, W, tile, o)
    s = {k: int(v) for k, v in zip(FIELDS, o)}
    return dict(s, name=so.st_name(s["kernel"]).decode())


def restated_rows(tile, budget):
    rows = budget // tile
    if tile > 1:
        rows = min(rows, (2 ** 32 - 1) // (tile * (tile - 1) // 2))
    return max(1, min(rows, tile))


def test_select_constants_and_names(sel):
    Kc = {n: sel.st_const(i) for i, n in enumerate(CONSTS)}
    assert (Kc["TPB"], Kc["MAX_CLASSES"], Kc["WG_BYTES"], Kc["MAX_GRID"], Kc["MAX_SIDE"]) == (256, 64, 65536, 1 << 20, 32768)
    assert sel.st_const(len(CONSTS)) == -1 and sel.st_count() == 2
    assert [sel.st_name(k).decode() for k in range(2)] == ["seg_class_stats_kernel<1>", "seg_class_stats_kernel<16>"]
    assert sel.st_name(2) is None and sel.st_name(-1) is None
    assert sel.st_classes_ok(1) and sel.st_classes_ok(64) and not sel.st_classes_ok(0) and not sel.st_classes_ok(65)


def test_16_byte_loads_only_for_aligned_labels_and_w_and_tile_multiples_of_16(sel):
    assert select(sel, 1, 1024, 2048, 1024)["name"] == "seg_class_stats_kernel<16>" and select(sel, 1, 1024, 2048, 1024)["vec"] == 16
    assert select(sel, 1, 1024, 2048, 1024, off=1)["vec"] == 1 and select(sel, 1, 1024, 2048, 1024, off=8)["vec"] == 1
    assert select(sel, 1, 1024, 2048, 1024, off=16)["vec"] == 16 and select(sel, 1, 1024, 2048, 1024, off=1)["name"] == "seg_class_stats_kernel<1>"
    assert select(sel, 2, 64, 160, 32)["vec"] == 16 and select(sel, 2, 64, 168, 32)["vec"] == 1, "W % 16"
    assert select(sel, 2, 64, 160, 16)["vec"] == 16 and select(sel, 2, 64, 160, 24)["vec"] == 1 and select(sel, 2, 64, 160, 8)["vec"] == 1, "tile % 16"
    for width in (72, 44):
        for tile in TILES:
            assert select(sel, 4, 40, width, tile)["vec"] == 1, "the fixture maps: 72 and 44 are no multiples of 16"
    assert select(sel, 2, 300, 520, 256)["vec"] == 1 and select(sel, 1, 4096, 4096, 4096)["vec"] == 16


def test_rows_per_workgroup_on_both_sides_of_the_byte_budget_and_of_the_uint32_bound(sel):
    budget = sel.st_const(CONSTS.index("WG_BYTES"))
    for tile in (1, 2, 8, 16, 20, 40, 255, 256, 257, 1024, 4096, 8192, 16384, 32768):
        assert sel.st_rows(tile, budget) == restated_rows(tile, budget) and select(sel, 1, 32768, 32768, tile)["rows"] == restated_rows(tile, budget)
    assert sel.st_rows(256, budget) == 256 and sel.st_rows(257, budget) == 255, "a whole tile while it fits the budget"
    assert sel.st_rows(1024, budget) == 64 and sel.st_rows(32768, budget) == 2 and sel.st_rows(32768, 1) == 1
    # at the shipped budget the byte budget is always the tighter limit; a larger budget meets the bound rows * tile * (tile - 1) / 2 < 2^32
    for tile in range(2, 32769, 509):
        assert sel.st_rows(tile, budget) * (tile * (tile - 1) // 2) < 2 ** 32
    big = 1 << 30
    assert sel.st_rows(4096, big) == 512 == (2 ** 32 - 1) // (4096 * 4095 // 2) and 513 * (4096 * 4095 // 2) >= 2 ** 32, "the bound binds: 512 rows, not 4096"
    assert sel.st_rows(4096, 511 * 4096) == 511 and sel.st_rows(4096, 512 * 4096) == 512 and sel.st_rows(4096, 513 * 4096) == 512
    assert sel.st_rows(32768, big) == 8 and sel.st_rows(2048, big) == 2048, "tile 2048: 2048 rows sum to 2^32 - 2^21, the whole tile fits"
    assert sel.st_rows(2896, big) == 1024 and sel.st_rows(2897, big) == 1023
    for tile in (2048, 2896, 2897, 4096, 32768):
        r = sel.st_rows(tile, big)
        assert r == restated_rows(tile, big) and r * (tile * (tile - 1) // 2) < 2 ** 32 and tile * r * (r - 1) // 2 < 2 ** 32


def test_the_grid_covers_every_row_of_every_tile_once_and_is_capped(sel):
    s = select(sel, 2975, 1024, 2048, 1024)
    assert (s["th"], s["tw"], s["rows"], s["chunks"], s["units"], s["grid"], s["launch"]) == (1, 2, 64, 16, 2975 * 2 * 16, 2975 * 2 * 16, 1)
    s = select(sel, 2, 300, 520, 256)
    assert (s["th"], s["tw"], s["rows"], s["chunks"], s["units"], s["grid"]) == (1, 2, 256, 1, 4, 4)
    s = select(sel, 1, 4096, 4096, 4096)
    assert (s["rows"], s["chunks"], s["units"]) == (16, 256, 256)
    s = select(sel, 4, 40, 72, 8)
    assert (s["th"], s["tw"], s["rows"], s["chunks"], s["units"]) == (5, 9, 8, 1, 180)
    s = select(sel, 2975, 1024, 2048, 8)
    assert s["units"] == 2975 * 128 * 256 and s["grid"] == 1 << 20, "more units than workgroups: the kernel walks them"
    for H, W, tile in ((40, 72, 64), (40, 72, 41), (72, 40, 64), (1, 1, 2)):
        s = select(sel, 4, H, W, tile)
        assert s["launch"] == 0 and s["units"] == 0 and s["grid"] == 0, "a tile larger than the image: nothing to launch"
    assert select(sel, 4, 40, 72, 40)["launch"] == 1


def test_the_selection_header_is_plain_host_code_and_the_launcher_notes_its_names():
    with open(os.path.join(CSRC, "seg_stats_select.h")) as f:
        code = re.sub(r"//.*", "", f.read())
    assert "hip" not in code.lower() and "getenv" not in code
    with open(os.path.join(CSRC, "seg_stats_ops.hip")) as f:
        src = f.read()
    assert src.count("KD_NOTE_PLUMBING(seg_stats_kernel_name(sel.kernel))") == 1 and src.count("seg_stats_select(") == 1
    assert "& 15" not in src and "aligned16" not in src and "% 16" not in src, "the launcher decides nothing itself"


def test_the_sweep_program_builds_and_runs_clean():
    """tests/seg_stats_select_host/sweep_main.cpp, a program of its own, without the sanitizers (`make sweep` adds them)."""
    subprocess.check_call(["make", "-s", "-C", WRAP, "_build/sweep_plain"])
    out = subprocess.run([os.path.join(WRAP, "_build", "sweep_plain")], capture_output=True, text=True)
    assert out.returncode == 0 and "no finding" in out.stdout, out.stderr
