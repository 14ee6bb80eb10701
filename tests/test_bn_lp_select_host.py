"""The bf16 NHWC BatchNorm selection the library really runs (csrc/bn_lp_select.h: the vector gate, the grids, the workspace), compiled
for the host -- without a GPU.  Both sides of the vector gate on each operand alone (C % 8, a 2-byte base offset, a leading
dimension whose bytes are no multiple of 16); an absent operand never in the way; the grid at its cap and one item over it; the
workspace against the library's kd_bn_nhwc_lp_workspace (and the fp32 entry points', whose finish kernel the forward shares); the
name table and the header's hygiene."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "bn_lp_select_host")
CSRC = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
FIELDS = ("kernel", "vec", "nrb", "part_x", "part_y", "finish", "grid")
CONSTS = ("ROWS", "TPB", "CBLOCK", "VEC", "CAP", "FWD_FINISH_CH", "BWD_FINISH_CH")
BASE = 0x10000           # a buffer's base (the allocator's are 256-B aligned)
i32, i64, u64, out = C.c_int, C.c_longlong, C.c_ulonglong, C.POINTER(C.c_double)
OPERANDS = ("gy", "x", "y", "res", "dx")


def load():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libbn_lp_select.so"))
    so.bl_name.restype = C.c_char_p
    so.bl_const.restype = i64
    so.bl_grid.restype, so.bl_grid.argtypes = C.c_uint, [i64]
    so.bl_view_ok.argtypes = [i64, i32]
    so.bl_workspace.restype, so.bl_workspace.argtypes = u64, [i64, i32]
    so.bl_sums_offset.restype, so.bl_sums_offset.argtypes = u64, [i64, i32]
    so.bl_fwd.argtypes = [i64, i32] * 2 + [i64, i32, out]
    so.bl_bwd.argtypes = [i64, i32] * 5 + [i64, i32, out]
    return so


@pytest.fixture(scope="module")
def lib():
    return load()


def consts(lib):
    return {n: lib.bl_const(i) for i, n in enumerate(CONSTS)}


def call(lib, fn, *args):
    o = (C.c_double * len(FIELDS))()
    getattr(lib, "bl_" + fn)(*args, o)
    sel = {k: int(v) for k, v in zip(FIELDS, o)}
    sel["name"] = lib.bl_name(sel["kernel"]).decode()
    return sel


def bwd(lib, M, Cc, views):
    """views: operand -> (pointer value, ld); an operand that is not named is absent."""
    args = []
    for name in OPERANDS:
        args += list(views.get(name, (0, 0)))
    return call(lib, "bwd", *args, M, Cc)


def dense(Cc, *names):
    return {n: (BASE, Cc) for n in names}


# what takes a view off the vector path, each alone: (byte offset of the base, extra elements of ld)
OFF_PATH = {"a 2-byte base offset": (2, 0), "an 8-byte base offset": (8, 8), "ld * 2 % 16 != 0": (0, 1), "ld one 8-byte step on": (0, 4)}
ON_PATH = {"dense": (0, 0), "a 16-byte base offset in a wider buffer": (16, 8), "ld * 2 % 16 == 0": (0, 8)}


def test_the_view_predicate_on_both_sides():
    so = load()
    for off, ld in itertools.product((0, 2, 8, 16, 32), (64, 65, 68, 72)):
        assert bool(so.bl_view_ok(BASE + off, ld)) == (off % 16 == 0 and ld * 2 % 16 == 0), (off, ld)
    assert so.bl_view_ok(0, 65), "an absent operand never stands in the way"


def test_forward_vector_gate_on_each_operand_alone(lib):
    for Cc in (8, 64, 160):
        assert call(lib, "fwd", BASE, Cc, BASE, Cc, 100, Cc)["name"] == "bn_lp_apply_kernel<8>"
        for who in (0, 1):
            for why, (off, pad) in OFF_PATH.items():
                v = [(BASE, Cc), (BASE, Cc)]
                v[who] = (BASE + off, Cc + pad)
                sel = call(lib, "fwd", *v[0], *v[1], 100, Cc)
                assert sel["name"] == "bn_lp_apply_kernel<1>" and not sel["vec"], (Cc, who, why)
            for why, (off, pad) in ON_PATH.items():
                v = [(BASE, Cc), (BASE, Cc)]
                v[who] = (BASE + off, Cc + pad)
                sel = call(lib, "fwd", *v[0], *v[1], 100, Cc)
                assert sel["name"] == "bn_lp_apply_kernel<8>" and sel["vec"], (Cc, who, why)
    for Cc in (1, 6, 12, 65):     # C % 8 alone, on aligned dense views (12 * 2 B = 24 B: the ld gate would catch it too; 6, 65 likewise)
        assert call(lib, "fwd", BASE, 72, BASE, 72, 100, Cc)["name"] == "bn_lp_apply_kernel<1>"
    assert call(lib, "fwd", BASE, 72, BASE + 16, 72, 100, 64)["name"] == "bn_lp_apply_kernel<8>"      # the GPU test's ld-72 slice at offset 8
    assert call(lib, "fwd", BASE, 65, BASE, 65, 100, 64)["name"] == "bn_lp_apply_kernel<1>"           # ... and its ld-65 one


def test_backward_vector_gate_on_each_operand_alone_and_absent_operands(lib):
    Cc, M = 64, 300
    full = dense(Cc, *OPERANDS)
    assert bwd(lib, M, Cc, full)["name"] == "bn_lp_dx_kernel<8>"
    for who in OPERANDS:
        for why, (off, pad) in OFF_PATH.items():
            v = dict(full)
            v[who] = (BASE + off, Cc + pad)
            sel = bwd(lib, M, Cc, v)
            assert sel["name"] == "bn_lp_dx_kernel<1>" and not sel["vec"], (who, why)
        for why, (off, pad) in ON_PATH.items():
            v = dict(full)
            v[who] = (BASE + off, Cc + pad)
            assert bwd(lib, M, Cc, v)["name"] == "bn_lp_dx_kernel<8>", (who, why)
    # an absent operand never blocks the vector path, whatever leading dimension comes with the null pointer
    for gone in itertools.chain.from_iterable(itertools.combinations(("y", "res", "dx"), n) for n in (1, 2, 3)):
        v = dict(full)
        for name in gone:
            v[name] = (0, 65)
        sel = bwd(lib, M, Cc, v)
        assert sel["vec"] and sel["name"] == ("bn_lp_grad_partial_kernel<8>" if "dx" in gone else "bn_lp_dx_kernel<8>"), gone
    # without dx the reduction alone: its variant still follows the operands it reads
    v = dense(Cc, "gy", "x", "y")
    assert bwd(lib, M, Cc, v)["name"] == "bn_lp_grad_partial_kernel<8>"
    v["x"] = (BASE + 2, Cc)
    assert bwd(lib, M, Cc, v)["name"] == "bn_lp_grad_partial_kernel<1>"
    assert bwd(lib, M, 6, dense(6, "gy", "x"))["name"] == "bn_lp_grad_partial_kernel<1>"
    assert bwd(lib, M, 6, dense(6, *OPERANDS))["name"] == "bn_lp_dx_kernel<1>"


def test_the_grids(lib):
    K = consts(lib)
    assert (K["ROWS"], K["TPB"], K["CBLOCK"], K["VEC"], K["CAP"], K["FWD_FINISH_CH"], K["BWD_FINISH_CH"]) == (128, 256, 64, 8, 8192, 16, 64)
    cap = K["CAP"]
    assert [lib.bl_grid(cap * 256 + d) for d in (-256, -255, -1, 0, 1)] == [cap - 1, cap, cap, cap, cap]
    assert [lib.bl_grid(t) for t in (-5, 0, 1, 256, 257)] == [1, 1, 1, 1, 2]
    # through the selectors: the cap exactly and one item over it, vector (a lane owns 8 channels) and scalar (C = 1, and C = 8 behind a
    # leading dimension of 9); (262145, 64) is the GPU test's over-cap row of the vector path
    for M, Cc, ld, vec, over in ((cap * 256, 8, 8, True, 0), (cap * 256 + 1, 8, 8, True, 1), (cap * 256, 1, 1, False, 0), (cap * 256 + 1, 1, 1, False, 1),
                                 (262144, 64, 64, True, 0), (262145, 64, 64, True, 8), (262144, 8, 9, False, 0), (262145, 8, 9, False, 8)):
        per = Cc // 8 if vec else Cc
        assert M * per == cap * 256 + over
        for sel in (call(lib, "fwd", BASE, ld, BASE, ld, M, Cc), bwd(lib, M, Cc, {n: (BASE, ld) for n in OPERANDS})):
            assert sel["vec"] == vec and sel["grid"] == cap
        short = call(lib, "fwd", BASE, ld, BASE, ld, M - 300, Cc)
        assert short["grid"] < cap and short["grid"] * 256 >= (M - 300) * per > (short["grid"] - 1) * 256
    # the two-stage reductions: 128 pixels x 64 channels a block; 16 (forward) / 64 (backward) channels per finishing block
    for M, Cc in itertools.product((1, 127, 128, 129, 2048, 2049), (6, 8, 64, 65, 160)):
        f, b = call(lib, "fwd", BASE, Cc, BASE, Cc, M, Cc), bwd(lib, M, Cc, dense(Cc, *OPERANDS))
        for sel, ch in ((f, 16), (b, 64)):
            assert (sel["nrb"], sel["part_x"], sel["part_y"], sel["finish"]) == (-(-M // 128), -(-M // 128), -(-Cc // 64), -(-Cc // ch)), (M, Cc)


def fp32_workspace(M, Cc):
    return (-(-M // 128) * 3 * Cc + 2 * Cc) * 4 if M > 0 and Cc > 0 else 0


def test_the_workspace_is_the_librarys():
    so = load()
    import kdcc_amd  # noqa: F401
    from kdcc_amd import _lib
    L = _lib.lib()
    for M, Cc in itertools.product((0, 1, 127, 128, 129, 2048, 2049, 262145, 2 ** 31 - 1), (0, 1, 6, 8, 64, 160, 640, 4096)):
        need = so.bl_workspace(M, Cc)
        assert need == L.kd_bn_nhwc_lp_workspace(M, Cc) == fp32_workspace(M, Cc) == L.kd_bn_nhwc_workspace(M, Cc), (M, Cc)
        if need:     # the backward's [row block][2][C] partials and the two sum rows behind the forward's [row block][3][C]
            assert so.bl_sums_offset(M, Cc) == -(-M // 128) * 3 * Cc and (so.bl_sums_offset(M, Cc) + 2 * Cc) * 4 == need


def test_the_names_are_distinct(lib):
    n = lib.bl_count()
    names = [lib.bl_name(k).decode() for k in range(n)]
    assert lib.bl_name(n) is None and lib.bl_name(-1) is None
    assert len(set(names)) == n == 6
    assert names == [f"bn_lp_{k}_kernel<{v}>" for k in ("apply", "dx", "grad_partial") for v in (1, 8)]


def test_the_selection_header_is_plain_host_code_and_the_launchers_note_its_names():
    with open(os.path.join(CSRC, "bn_lp_select.h")) as f:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
    assert not re.search(r"\bhip\w*|\bgetenv\b", text, flags=re.I)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", "<stdint.h>", '"../../include/kdcc.h"']
    with open(os.path.join(CSRC, "bn_nhwc_lp.hip")) as f:
        src = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
    assert not re.search(r'KD_NOTE_PLUMBING\(\s*"', src)
    assert re.findall(r"KD_NOTE_PLUMBING\(([^;]*)\);", src) == ["bn_lp_kernel_name(sel.kernel)"] * 2
    assert "vec4_ok" not in src and "grid_for" not in src and "aligned16" not in src, "the launchers decide nothing themselves"
