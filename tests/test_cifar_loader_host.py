"""kdcc_amd.data_loader without a GPU: the CIFAR-10 / CIFAR-100 files are parsed from disk (no torchvision, no download), the
validation split is the reference's numpy computation, lengths and the short last batch, the epoch's draws (a permutation, offsets
in 0..8, reproducible from the seed, other numbers the next epoch, every offset and flip reached), the host batches against the
per-image PIL oracle of tests/_cifar_loader_ref.py bit for bit in every layout and dtype, the config plug point, and the kernel
selection the library really runs (csrc/data_select.h compiled for the host) on both sides of every gate."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cifar_loader_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "data_select_host")
CSRC = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
BF = torch.bfloat16
LAYOUTS = ("nchw", "nhwc", "padded")
DTYPES = (torch.float32, BF)


@pytest.fixture(scope="module")
def c10(tmp_path_factory):
    """35 training images in five files of 7, and a test file of 7."""
    root = str(tmp_path_factory.mktemp("c10"))
    return (root,) + R.write_cifar10(root, 7)


@pytest.fixture(scope="module")
def c100(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("c100"))
    return (root,) + R.write_cifar100(root, 37, 6)


def loaders():
    from kdcc_amd import data_loader
    return data_loader


# ------------------------------------------------------------------------------------------------------------------ files
def test_both_formats_parse_without_torchvision_or_a_download(c10, c100):
    DL = loaders()
    root, tr, trl, te, tel = c10
    for training, imgs, labels in ((True, tr, trl), (False, te, tel)):
        L = DL.Cifar10Dataloader(root, 4, shuffle=False, training=training, device="cpu")
        assert len(L.dataset) == L.n_samples == len(imgs) and np.array_equal(L.dataset.data, imgs) and list(L.dataset.targets) == labels
        assert L.dataset.data.dtype == np.uint8 and L.dataset.data.shape[1:] == (32, 32, 3)
    root, tr, trl, te, tel = c100
    for training, imgs, labels in ((True, tr, trl), (False, te, tel)):
        L = DL.Cifar100Dataloader(root, 4, shuffle=False, num_workers=8, training=training, device="cpu")
        assert len(L.dataset) == len(imgs) and np.array_equal(L.dataset.data, imgs) and list(L.dataset.targets) == labels
        assert max(L.dataset.targets) > 9, "the fine labels, not the coarse ones"
    assert "torchvision" not in sys.modules
    assert (DL.Cifar10Dataloader.MEAN, DL.Cifar10Dataloader.STD) == (R.C10_MEAN, R.C10_STD), "the reference's quirk: ImageNet statistics"
    assert (DL.Cifar100Dataloader.MEAN, DL.Cifar100Dataloader.STD) == (R.C100_MEAN, R.C100_STD)


def test_a_missing_directory_is_named(tmp_path, c10):
    DL = loaders()
    with pytest.raises(FileNotFoundError, match="cifar-10-batches-py"):
        DL.Cifar10Dataloader(str(tmp_path), 4, device="cpu")
    with pytest.raises(FileNotFoundError, match="cifar-100-python"):
        DL.Cifar100Dataloader(str(tmp_path), 4, device="cpu")
    os.makedirs(tmp_path / "cifar-10-batches-py")
    with pytest.raises(FileNotFoundError, match="data_batch_1"):
        DL.Cifar10Dataloader(str(tmp_path), 4, device="cpu")
    with pytest.raises(ValueError):
        DL.Cifar10Dataloader(c10[0], 4, device="cpu", layout="chwn")
    with pytest.raises(TypeError):
        DL.Cifar10Dataloader(c10[0], 4, device="cpu", dtype=torch.float16)


# ------------------------------------------------------------------------------------------------------- split and lengths
def restated_split(n, split):
    idx = np.arange(n)
    np.random.seed(0)
    np.random.shuffle(idx)
    k = split if isinstance(split, int) else int(n * split)
    return idx[k:], idx[:k]


@pytest.mark.parametrize("split", [0.2, 0.1, 5, 36])
def test_the_split_is_the_references(c100, split):
    DL = loaders()
    L = DL.Cifar100Dataloader(c100[0], 5, shuffle=True, validation_split=split, device="cpu", seed=1)
    train, valid = restated_split(37, split)
    assert np.array_equal(L.sampler.indices, train) and np.array_equal(L.valid_sampler.indices, valid)
    assert L.shuffle is False and L.n_samples == len(train) and L.validation_split == split and len(L.dataset) == 37
    assert len(L) == -(-len(train) // 5)
    V = L.split_validation()
    assert V.n_samples == len(valid) and len(V) == -(-len(valid) // 5) and V.split_validation() is None and V.training
    got = torch.cat([t for _, t in V])
    assert sorted(V.epoch_params()[:, 0].tolist()) == sorted(valid.tolist()) and got.shape[0] == len(valid)
    assert V.epoch_params()[:, 1:3].unique().numel() > 1 or len(valid) < 4, "the validation loader of a training loader augments"
    list(L)
    assert sorted(L.epoch_params()[:, 0].tolist()) == sorted(train.tolist()), "a split loader walks its own indices, permuted"


def test_no_split_no_validation_loader_and_the_lengths(c10):
    DL = loaders()
    root, tr, trl = c10[:3]
    L = DL.Cifar10Dataloader(root, 5, shuffle=False, training=False, device="cpu")       # the 7-image test file
    assert L.split_validation() is None and L.sampler is None and L.valid_sampler is None and (len(L), L.batch_size) == (2, 5)
    L = DL.Cifar10Dataloader(root, 5, shuffle=True, device="cpu", seed=0)
    assert L.n_samples == 35 and len(L) == 7
    with pytest.raises(AssertionError):
        DL.Cifar10Dataloader(root, 5, validation_split=35, device="cpu")


def test_the_short_last_batch_of_37_images_in_fives(c100):
    DL = loaders()
    L = DL.Cifar100Dataloader(c100[0], 5, shuffle=True, device="cpu", seed=4)
    assert len(L) == 8
    sizes = [(tuple(x.shape), tuple(t.shape)) for x, t in L]
    assert sizes == [((5, 3, 32, 32), (5,))] * 7 + [((2, 3, 32, 32), (2,))]


# ---------------------------------------------------------------------------------------------------------------- sampling
def test_unshuffled_evaluation_is_the_files_order_unaugmented(c100):
    DL = loaders()
    root, _, _, te, tel = c100
    L = DL.Cifar100Dataloader(root, 4, shuffle=False, training=False, device="cpu")
    batches = list(L)
    p = L.epoch_params()
    assert p.dtype == torch.int32 and p.tolist() == [[i, 4, 4, 0] for i in range(len(te))]
    x = torch.cat([b for b, _ in batches])
    ref = torch.stack([R.oracle_image(te[i], 4, 4, 0, R.C100_MEAN, R.C100_STD) for i in range(len(te))])
    plain = torch.from_numpy(te).permute(0, 3, 1, 2).float().div(255)
    plain = plain.sub(torch.tensor(R.C100_MEAN).view(1, 3, 1, 1)).div(torch.tensor(R.C100_STD).view(1, 3, 1, 1))
    assert torch.equal(x, ref) and torch.equal(x, plain) and torch.cat([t for _, t in batches]).tolist() == tel


def test_the_epoch_table_is_a_seeded_permutation_with_offsets_in_range(c100):
    DL = loaders()
    mk = lambda seed, **kw: DL.Cifar100Dataloader(c100[0], 5, shuffle=True, device="cpu", seed=seed, **kw)
    A, B, Cc = mk(11), mk(11), mk(12)
    assert A.epoch_params() is None
    list(A), list(B), list(Cc)
    a1, b1, c1 = A.epoch_params(), B.epoch_params(), Cc.epoch_params()
    assert sorted(a1[:, 0].tolist()) == list(range(37)) and a1[:, 0].tolist() != list(range(37))
    assert 0 <= int(a1[:, 1:3].min()) and int(a1[:, 1:3].max()) <= 8 and set(a1[:, 3].tolist()) == {0, 1}
    assert torch.equal(a1, b1) and not torch.equal(a1, c1), "reproducible from the seed, other numbers from another"
    list(A), list(B)
    a2 = A.epoch_params()
    assert torch.equal(a2, B.epoch_params()) and not torch.equal(a1, a2) and sorted(a2[:, 0].tolist()) == list(range(37))
    # seed=None: the script's torch.manual_seed governs
    torch.manual_seed(77)
    D = mk(None)
    torch.manual_seed(77)
    E = mk(None)
    list(D), list(E)
    assert torch.equal(D.epoch_params(), E.epoch_params())
    # shuffle off, training on: the order stays, the augmentation is drawn
    F = DL.Cifar100Dataloader(c100[0], 5, shuffle=False, device="cpu", seed=1)
    list(F)
    assert F.epoch_params()[:, 0].tolist() == list(range(37)) and F.epoch_params()[:, 1:3].unique().numel() > 1


def test_every_offset_and_flip_occurs_on_4096_images(tmp_path):
    DL = loaders()
    R.write_cifar100(str(tmp_path), 4096, 1)
    L = DL.Cifar100Dataloader(str(tmp_path), 128, device="cpu", seed=2024)
    p = L._draw_epoch()
    assert sorted(p[:, 0].tolist()) == list(range(4096))
    seen = {(dy, dx, fl) for _, dy, dx, fl in p.tolist()}
    assert seen == set(itertools.product(range(9), range(9), range(2))), "81 offsets x 2 flips"


# ------------------------------------------------------------------------------------------------------------ host batches
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_host_batches_equal_the_pil_oracle_bit_for_bit(c10, c100, layout, dtype):
    DL = loaders()
    from kdcc_amd import nn_hip
    for cls, (root, tr, trl, _, _), mean, std in ((DL.Cifar10Dataloader, c10, R.C10_MEAN, R.C10_STD),
                                                  (DL.Cifar100Dataloader, c100, R.C100_MEAN, R.C100_STD)):
        L = cls(root, 5, device="cpu", dtype=dtype, layout=layout, seed=0)
        table = R.extreme_params(len(tr), 40)
        got = list(L.batches(table))
        assert torch.equal(L.epoch_params(), table) and [b.shape[0] for b, _ in got] == [5] * 8
        ref_x, ref_y = R.oracle_batch(tr, trl, table, mean, std, dtype)
        assert torch.equal(torch.cat([R.logical(b) for b, _ in got]), ref_x) and torch.equal(torch.cat([t for _, t in got]), ref_y)
        b = got[0][0]
        assert b.dtype == dtype and tuple(b.shape) == (5, 3, 32, 32) and b.device.type == "cpu"
        G = nn_hip._granule_up(3, dtype)
        if layout == "nchw":
            assert b.is_contiguous()
        elif layout == "nhwc":
            assert b.is_contiguous(memory_format=torch.channels_last) and getattr(b, nn_hip._PADDED, 0) == 0
        else:
            assert G == (32 if dtype == torch.float32 else 64) and getattr(b, nn_hip._PADDED) == G and b.stride() == (1024 * G, 1, 32 * G, G)
            whole = b.permute(0, 2, 3, 1).as_strided((5, 32, 32, G), (1024 * G, 32 * G, G, 1))
            assert not bool(whole[..., 3:].any()) and torch.equal(whole[..., :3].permute(0, 3, 1, 2), b)
        # a drawn epoch too: the table it reports is the table it used
        batches = list(L)
        ref_x, ref_y = R.oracle_batch(tr, trl, L.epoch_params(), mean, std, dtype)
        assert torch.equal(torch.cat([R.logical(x) for x, _ in batches]), ref_x) and torch.equal(torch.cat([t for _, t in batches]), ref_y)


def test_a_table_out_of_range_is_refused_on_the_host(c100):
    DL = loaders()
    L = DL.Cifar100Dataloader(c100[0], 5, device="cpu", seed=0)
    for bad in ([37, 4, 4, 0], [-1, 4, 4, 0], [0, 9, 4, 0], [0, 4, -1, 0], [0, 4, 4, 2]):
        with pytest.raises(ValueError):
            L.batches(torch.tensor([[0, 0, 0, 0], bad], dtype=torch.int32))
    with pytest.raises(ValueError):
        L.batches(torch.zeros((3, 3), dtype=torch.int32))


def test_the_table_is_torchvisions_arithmetic():
    from kdcc_amd.base.base_data_loader import normalisation_table
    t = normalisation_table(R.C10_MEAN, R.C10_STD)
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    x = torch.from_numpy(img).permute(2, 0, 1).contiguous().float().div(255)
    x = x.sub_(torch.tensor(R.C10_MEAN).view(3, 1, 1)).div_(torch.tensor(R.C10_STD).view(3, 1, 1))
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 256) and torch.equal(t, x.reshape(3, 256))
    assert torch.equal(normalisation_table(R.C10_MEAN, R.C10_STD, BF), t.to(BF))


# ---------------------------------------------------------------------------------------------------------- the plug point
def reference_config(root, kind, save_dir):
    from _netutil import trainer_config
    cfg = trainer_config([], lr=0.1, len_epoch=2, save_dir=save_dir)
    cfg["train_data_loader"] = {"type": kind, "args": {"data_dir": root, "batch_size": 8, "shuffle": True, "validation_split": 0.1, "num_workers": 0}}
    cfg["test_data_loader"] = {"type": kind, "args": {"data_dir": root, "batch_size": 8, "shuffle": False, "validation_split": 0.0, "num_workers": 0,
                                                      "training": False}}
    return cfg


def test_the_config_resolves_both_loaders(c10, c100, tmp_path):
    import kdcc_amd
    from kdcc_amd import ConfigParser, base
    for kind, (root, tr, _, te, _) in (("Cifar10Dataloader", c10), ("Cifar100Dataloader", c100)):
        config = ConfigParser(reference_config(root, kind, str(tmp_path / kind)), run_id=kind)
        L = config.init_obj("train_data_loader", kdcc_amd.data_loader, device="cpu")
        assert type(L).__name__ == kind and isinstance(L, base.BaseDataLoader) and L.batch_size == 8
        assert L.n_samples == len(tr) - int(len(tr) * 0.1) and L.split_validation().n_samples == int(len(tr) * 0.1)
        T = config.init_obj("test_data_loader", kdcc_amd.data_loader, device="cpu")
        assert T.n_samples == len(te) and not T.training
        x, t = next(iter(L))
        assert tuple(x.shape) == (8, 3, 32, 32) and x.dtype == torch.float32 and t.dtype == torch.int64


# ----------------------------------------------------------------------------------------------------------- data_select.h
FIELDS = ("kernel", "vec", "elems", "items", "grid")
CONSTS = ("TPB", "SIDE", "CH", "PIXELS", "PAD", "VEC_BYTES", "MAX_ELEMS", "NCHW", "NHWC")
BASE = 0x10000
F32, BF16, NCHW, NHWC = 0, 1, 0, 1


@pytest.fixture(scope="module")
def sel():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libdata_select.so"))
    so.ds_name.restype = C.c_char_p
    so.ds_const.restype = so.ds_elems.restype = C.c_longlong
    so.ds_select.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_double)]
    return so


def select(so, dtype, layout, off, B, ld):
    o = (C.c_double * len(FIELDS))()
    so.ds_select(dtype, layout, BASE + off, B, ld, o)
    s = {k: int(v) for k, v in zip(FIELDS, o)}
    s["name"] = so.ds_name(s["kernel"]).decode()
    return s


def test_selection_constants_and_names(sel):
    K = {n: sel.ds_const(i) for i, n in enumerate(CONSTS)}
    assert K == dict(TPB=256, SIDE=32, CH=3, PIXELS=1024, PAD=4, VEC_BYTES=16, MAX_ELEMS=2 ** 31, NCHW=0, NHWC=1) and sel.ds_const(len(CONSTS)) == -1
    from kdcc_amd import _lib
    assert (_lib.KD_CIFAR_NCHW, _lib.KD_CIFAR_NHWC, _lib.KD_F32, _lib.KD_BF16) == (NCHW, NHWC, F32, BF16)
    n = sel.ds_count()
    names = [sel.ds_name(k).decode() for k in range(n)]
    assert sel.ds_name(n) is None and sel.ds_name(-1) is None and len(set(names)) == n == 8
    assert names == [f"cifar_batch_kernel<{d},{l},{v}>" for d, w in (("f32", 4), ("bf16", 8)) for l in ("nchw", "nhwc") for v in (1, w)]


def test_the_dtype_the_layout_and_the_base_alignment_each_alone(sel):
    B, ld = 5, 64
    for dtype, dn, w in ((F32, "f32", 4), (BF16, "bf16", 8)):
        for layout, ln in ((NCHW, "nchw"), (NHWC, "nhwc")):
            for off in (0, 16, 32, 4096):                   # every 16-byte aligned base stores 16 bytes at a time ...
                s = select(sel, dtype, layout, off, B, ld)
                assert s["name"] == f"cifar_batch_kernel<{dn},{ln},{w}>" and s["vec"] == w, (dn, ln, off)
            for off in (2, 4, 6, 8, 12, 14, 18):            # ... and no other does (2, 6, 14, 18: a bf16 element's alignment only)
                s = select(sel, dtype, layout, off, B, ld)
                assert s["name"] == f"cifar_batch_kernel<{dn},{ln},1>" and s["vec"] == 1, (dn, ln, off)
    # the pixel stride never moves the choice (the kernel owns the whole stride: the storage is one dense run), only the work
    for ld in (3, 4, 5, 7, 32, 33, 64):
        assert select(sel, BF16, NHWC, 0, 5, ld)["name"] == "cifar_batch_kernel<bf16,nhwc,8>"
        assert select(sel, F32, NHWC, 4, 5, ld)["name"] == "cifar_batch_kernel<f32,nhwc,1>"
        assert select(sel, F32, NHWC, 0, 5, ld)["elems"] == 5 * 1024 * ld == sel.ds_elems(NHWC, 5, ld)
        assert select(sel, F32, NCHW, 0, 5, ld)["elems"] == 5 * 3072 == sel.ds_elems(NCHW, 5, ld), "NCHW ignores ld"


def test_the_grid_covers_the_pieces_exactly(sel):
    for dtype, w in ((F32, 4), (BF16, 8)):
        for layout, B, ld, off in itertools.product((NCHW, NHWC), (1, 2, 5, 128, 129), (3, 5, 32, 64), (0, 4)):
            s = select(sel, dtype, layout, off, B, ld)
            v = w if off == 0 else 1
            elems = B * 1024 * (ld if layout == NHWC else 3)
            assert (s["vec"], s["elems"], s["items"], s["grid"]) == (v, elems, elems // v, -(-(elems // v) // 256))
            assert s["items"] * v == elems and s["items"] >= B, "whole pieces, and a thread for every label"
    # one piece over a block boundary: B = 1, ld = 3 in bf16 is 384 pieces = 1.5 blocks; fp32 ld = 5, B = 1: 1280 pieces = 5 blocks
    assert select(sel, BF16, NHWC, 0, 1, 3)["grid"] == 2 and select(sel, F32, NHWC, 0, 1, 5)["grid"] == 5


def test_the_argument_predicates_on_both_sides(sel):
    assert [bool(sel.ds_dtype_ok(d)) for d in (-1, 0, 1, 2)] == [False, True, True, False]
    assert [bool(sel.ds_layout_ok(l)) for l in (-1, 0, 1, 2)] == [False, True, True, False]
    assert [bool(sel.ds_shape_ok(NHWC, B, 3)) for B in (-1, 0, 1)] == [False, False, True]
    assert [bool(sel.ds_shape_ok(NHWC, 1, ld)) for ld in (-3, 0, 2, 3)] == [False, False, False, True]
    assert bool(sel.ds_shape_ok(NCHW, 1, 0)) and bool(sel.ds_shape_ok(NCHW, 1, -7)), "NCHW ignores ld"
    # 2^31 elements at most: NCHW 3072 an image, padded bf16 65536 an image
    assert [bool(sel.ds_shape_ok(NCHW, B, 3)) for B in (699050, 699051)] == [True, False]
    assert [bool(sel.ds_shape_ok(NHWC, B, 64)) for B in (32768, 32769)] == [True, False]
    assert [bool(sel.ds_shape_ok(NHWC, 1, ld)) for ld in (2 ** 21, 2 ** 21 + 1, 2 ** 31 - 1)] == [True, False, False]
    assert not sel.ds_shape_ok(NHWC, 2 ** 31 - 1, 2 ** 31 - 1)


def test_the_selection_header_is_plain_host_code_and_the_launcher_notes_its_names():
    with open(os.path.join(CSRC, "data_select.h")) as f:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
    assert not re.search(r"\bhip\w*|\bgetenv\b", text, flags=re.I)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", "<stdint.h>", '"../../include/kdcc.h"']
    with open(os.path.join(CSRC, "data_ops.hip")) as f:
        src = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
    assert not re.search(r'KD_NOTE_PLUMBING\(\s*"', src) and not re.search(r"\bgetenv\b", src)
    assert re.findall(r"KD_NOTE_PLUMBING\(([^;]*)\);", src) == ["data_kernel_name(sel.kernel)"]
    assert src.count("data_select(") == 1 and "& 15" not in src and "aligned16" not in src, "the launcher decides nothing itself"


def test_the_sweep_program_builds_and_runs_clean():
    """tests/data_select_host/sweep_main.cpp, a program of its own, without the sanitizers (`make sweep` adds them)."""
    subprocess.check_call(["make", "-s", "-C", WRAP, "_build/sweep_plain"])
    exe = os.path.join(WRAP, "_build", "sweep_plain")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "no finding" in out.stdout, out.stderr[-2000:]


def test_the_library_refuses_bad_arguments_before_any_launch():
    """kd_cifar_batch checks its arguments on the host: every refusal below returns before a launch (no GPU here)."""
    from kdcc_amd import _lib
    L = _lib.lib()
    p = 0x10000                                 # never dereferenced: each call is refused first

    def rc(data=p, labels=p, n=10, params=p, B=2, table=p, dtype=F32, layout=NHWC, out=p, ld=3, labels_out=p):
        return L.kd_cifar_batch(data, labels, n, params, B, table, dtype, layout, out, ld, labels_out, None)
    for name in ("data", "labels", "params", "table", "out", "labels_out"):
        assert rc(**{name: None}) == -1, name
    assert rc(dtype=2) == -1 and rc(layout=2) == -1 and rc(n=0) == -1 and rc(B=0) == -1 and rc(ld=2) == -1
    assert rc(out=p + 2) == -1 and rc(out=p + 1, dtype=BF16) == -1 and rc(params=p + 2) == -1, "operands aligned to their elements"
    assert rc(B=32769, ld=64) == _lib.KD_ERR_UNSUPPORTED and b"2^31" in L.kd_last_error()
