"""The NHWC BatchNorm selection the library really runs (csrc/bn_select.h: the vector gate, the grids, the workspace), compiled for
the host -- without a GPU -- at both element sizes: es = 2 (bf16, 8 channels a lane) and es = 4 (fp32, 4 channels a lane).  Both
sides of the vector gate on each operand alone (C % V, a base offset, a leading dimension whose bytes are no multiple of 16); an
absent operand never in the way; the stage-1 partials vector for bf16 only; the grid at its cap and one item over it; the
workspace against the library's kd_bn_nhwc_lp_workspace and kd_bn_nhwc_workspace; the name table and the header's hygiene."""
import itertools
import os
import re

import pytest

from _bn_select_host import BASE, OPERANDS, bwd, call, load

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
CONSTS = ("ROWS", "TPB", "CBLOCK", "VEC_BYTES", "CAP", "FWD_FINISH_CH", "BWD_FINISH_CH")
P = {2: "bn_lp", 4: "bn_nhwc"}      # the prefix of the noted names, by element size
V = {2: 8, 4: 4}                    # channels a lane of the vector kernels owns: 16 B


@pytest.fixture(scope="module")
def lib():
    return load()


def consts(lib):
    return {n: lib.bl_const(i) for i, n in enumerate(CONSTS)}


def dense(Cc, *names):
    return {n: (BASE, Cc) for n in names}


# what takes a view off the vector path, each alone: (byte offset of the base, extra elements of ld)
OFF_PATH = {2: {"a 2-byte base offset": (2, 0), "an 8-byte base offset": (8, 8), "ld * 2 % 16 != 0": (0, 1), "ld one 8-byte step on": (0, 4)},
            4: {"a 4-byte base offset": (4, 0), "an 8-byte base offset": (8, 4), "ld % 4 != 0": (0, 1), "ld one 8-byte step on": (0, 2)}}
ON_PATH = {2: {"dense": (0, 0), "a 16-byte base offset in a wider buffer": (16, 8), "ld * 2 % 16 == 0": (0, 8)},
           4: {"dense": (0, 0), "a 16-byte base offset in a wider buffer": (16, 4), "ld % 4 == 0": (0, 4)}}


def test_the_view_predicate_on_both_sides():
    so = load()
    for off, ld in itertools.product((0, 2, 8, 16, 32), (64, 65, 68, 72)):
        assert bool(so.bl_view_ok(2, BASE + off, ld)) == (off % 16 == 0 and ld * 2 % 16 == 0), (off, ld)
    for off, ld in itertools.product((0, 4, 8, 16, 32), (64, 65, 66, 68)):
        assert bool(so.bl_view_ok(4, BASE + off, ld)) == (off % 16 == 0 and ld % 4 == 0), (off, ld)
    assert so.bl_view_ok(2, 0, 65) and so.bl_view_ok(4, 0, 65), "an absent operand never stands in the way"


def test_forward_vector_gate_on_each_operand_alone(lib):
    for es in (2, 4):
        forward_gate(lib, es)


def forward_gate(lib, es):
    one, vec = f"{P[es]}_apply_kernel<1>", f"{P[es]}_apply_kernel<{V[es]}>"
    for Cc in (8, 64, 160):
        assert call(lib, "fwd", es, BASE, Cc, BASE, Cc, 100, Cc)["name"] == vec
        for who in (0, 1):
            for why, (off, pad) in OFF_PATH[es].items():
                v = [(BASE, Cc), (BASE, Cc)]
                v[who] = (BASE + off, Cc + pad)
                sel = call(lib, "fwd", es, *v[0], *v[1], 100, Cc)
                assert sel["name"] == one and not sel["vec"] and not sel["part_vec"], (Cc, who, why)
                assert not lib.bl_vec_ok(es, Cc, *v[0], *v[1])
            for why, (off, pad) in ON_PATH[es].items():
                v = [(BASE, Cc), (BASE, Cc)]
                v[who] = (BASE + off, Cc + pad)
                sel = call(lib, "fwd", es, *v[0], *v[1], 100, Cc)
                assert sel["name"] == vec and sel["vec"], (Cc, who, why)
                assert lib.bl_vec_ok(es, Cc, *v[0], *v[1])
    # C % V alone, on aligned views of ld 72 (72 * 2 B and 72 * 4 B are multiples of 16)
    for Cc in {2: (1, 6, 12, 65), 4: (1, 6, 10, 65)}[es]:
        assert call(lib, "fwd", es, BASE, 72, BASE, 72, 100, Cc)["name"] == one
    assert call(lib, "fwd", es, BASE, 72, BASE + 16, 72, 100, 64)["name"] == vec      # the GPU test's ld-72 slice at byte offset 16
    assert call(lib, "fwd", es, BASE, 65, BASE, 65, 100, 64)["name"] == one           # ... and its ld-65 one
    if es == 4:         # 4 channels are a vector of fp32 and none of bf16
        assert call(lib, "fwd", 4, BASE, 4, BASE, 4, 100, 4)["name"] == vec and not call(lib, "fwd", 2, BASE, 4, BASE, 4, 100, 4)["vec"]


def test_backward_vector_gate_on_each_operand_alone_and_absent_operands(lib):
    for es in (2, 4):
        backward_gate(lib, es)


def backward_gate(lib, es):
    Cc, M = 64, 300
    dx1, dxv = f"{P[es]}_dx_kernel<1>", f"{P[es]}_dx_kernel<{V[es]}>"
    # without dx: the bf16 partials follow the gate; the fp32 ones are scalar always, and the call is noted by its finish kernel
    grad1, gradv = ("bn_lp_grad_partial_kernel<1>", "bn_lp_grad_partial_kernel<8>") if es == 2 else ("bn_nhwc_grad_finish_kernel",) * 2
    full = dense(Cc, *OPERANDS)
    assert bwd(lib, es, M, Cc, full)["name"] == dxv
    for who in OPERANDS:
        for why, (off, pad) in OFF_PATH[es].items():
            v = dict(full)
            v[who] = (BASE + off, Cc + pad)
            sel = bwd(lib, es, M, Cc, v)
            assert sel["name"] == dx1 and not sel["vec"], (who, why)
        for why, (off, pad) in ON_PATH[es].items():
            v = dict(full)
            v[who] = (BASE + off, Cc + pad)
            assert bwd(lib, es, M, Cc, v)["name"] == dxv, (who, why)
    # an absent operand never blocks the vector path, whatever leading dimension comes with the null pointer
    for gone in itertools.chain.from_iterable(itertools.combinations(("y", "res", "dx"), n) for n in (1, 2, 3)):
        v = dict(full)
        for name in gone:
            v[name] = (0, 65)
        sel = bwd(lib, es, M, Cc, v)
        assert sel["vec"] and sel["name"] == (gradv if "dx" in gone else dxv), gone
    # without dx the reduction alone: its variant still follows the operands it reads
    v = dense(Cc, "gy", "x", "y")
    assert bwd(lib, es, M, Cc, v)["name"] == gradv
    v["x"] = (BASE + es, Cc)
    assert bwd(lib, es, M, Cc, v)["name"] == grad1
    assert bwd(lib, es, M, 6, dense(6, "gy", "x"))["name"] == grad1
    assert bwd(lib, es, M, 6, dense(6, *OPERANDS))["name"] == dx1


def test_the_partials_are_vector_for_bf16_only(lib):
    """part_vec is false for every fp32 call and equals vec for every bf16 call."""
    seen = set()
    for es, Cc, (off, pad), M in itertools.product((2, 4), (1, 4, 6, 8, 64, 65, 160), ((0, 0), (2, 0), (4, 0), (8, 4), (16, 8), (0, 1), (0, 2), (0, 4)),
                                                   (1, 129, 2049)):
        views = dense(Cc, *OPERANDS)
        for who in OPERANDS:
            v = dict(views)
            v[who] = (BASE + off, Cc + pad)
            sels = [bwd(lib, es, M, Cc, v), bwd(lib, es, M, Cc, {k: v[k] for k in ("gy", "x", "y")})]
            if who in ("x", "y"):
                sels.append(call(lib, "fwd", es, *v["x"], *v["y"], M, Cc))
            for sel in sels:
                assert sel["part_vec"] == (sel["vec"] if es == 2 else 0), (es, Cc, off, pad, who)
                seen.add((es, sel["vec"]))
    assert seen == {(2, 0), (2, 1), (4, 0), (4, 1)}


def test_the_grids(lib):
    K = consts(lib)
    assert (K["ROWS"], K["TPB"], K["CBLOCK"], K["VEC_BYTES"], K["CAP"], K["FWD_FINISH_CH"], K["BWD_FINISH_CH"]) == (128, 256, 64, 16, 8192, 16, 64)
    cap = K["CAP"]
    assert [lib.bl_grid(cap * 256 + d) for d in (-256, -255, -1, 0, 1)] == [cap - 1, cap, cap, cap, cap]
    assert [lib.bl_grid(t) for t in (-5, 0, 1, 256, 257)] == [1, 1, 1, 1, 2]
    # through the selectors: the cap exactly and one item over it, vector (a lane owns 16 B) and scalar (C = 1, and C = 8 behind a
    # leading dimension of 9); (262145, 64) is the GPU test's over-cap row of the bf16 vector path, M * C / 4 == 8192 * 256 (+ 1) the
    # fp32 one's
    rows = {2: ((cap * 256, 8, 8, True, 0), (cap * 256 + 1, 8, 8, True, 1), (cap * 256, 1, 1, False, 0), (cap * 256 + 1, 1, 1, False, 1),
                (262144, 64, 64, True, 0), (262145, 64, 64, True, 8), (262144, 8, 9, False, 0), (262145, 8, 9, False, 8)),
            4: ((cap * 256, 4, 4, True, 0), (cap * 256 + 1, 4, 4, True, 1), (cap * 256, 1, 1, False, 0), (cap * 256 + 1, 1, 1, False, 1),
                (131072, 64, 64, True, 0), (131073, 64, 64, True, 16), (262144, 8, 9, False, 0), (262145, 8, 9, False, 8))}
    for es in (2, 4):
        for M, Cc, ld, vec, over in rows[es]:
            per = Cc // V[es] if vec else Cc
            assert M * per == cap * 256 + over
            for sel in (call(lib, "fwd", es, BASE, ld, BASE, ld, M, Cc), bwd(lib, es, M, Cc, {n: (BASE, ld) for n in OPERANDS})):
                assert sel["vec"] == vec and sel["grid"] == cap
            short = call(lib, "fwd", es, BASE, ld, BASE, ld, M - 300, Cc)
            assert short["grid"] < cap and short["grid"] * 256 >= (M - 300) * per > (short["grid"] - 1) * 256
        # the two-stage reductions: 128 pixels x 64 channels a block; 16 (forward) / 64 (backward) channels per finishing block
        for M, Cc in itertools.product((1, 127, 128, 129, 2048, 2049), (6, 8, 64, 65, 160)):
            f, b = call(lib, "fwd", es, BASE, Cc, BASE, Cc, M, Cc), bwd(lib, es, M, Cc, dense(Cc, *OPERANDS))
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
    assert len(set(names)) == n == 11
    assert names == ([f"bn_nhwc_{k}_kernel<{v}>" for k in ("apply", "dx") for v in (1, 4)] + ["bn_nhwc_grad_finish_kernel"]
                     + [f"bn_lp_{k}_kernel<{v}>" for k in ("apply", "dx", "grad_partial") for v in (1, 8)])


def test_the_selection_header_is_plain_host_code_and_the_launchers_note_its_names():
    def code(name):
        with open(os.path.join(CSRC, name)) as f:
            return re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
    text = code("bn_select.h")
    assert not re.search(r"\bhip\w*|\bgetenv\b", text, flags=re.I)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", "<stdint.h>", '"../../include/kdcc.h"']
    assert sorted(n for n in os.listdir(CSRC) if n.startswith("bn_")) == ["bn_nhwc.hip", "bn_nhwc_core.h", "bn_select.h"]
    # bn_nhwc.hip only casts and calls; the implementations it calls (bn_nhwc_core.h) and dense_ops.hip note the table's names
    notes = {name: re.findall(r"KD_NOTE_PLUMBING\(([^;]*)\);", code(name)) for name in ("bn_nhwc.hip", "bn_nhwc_core.h", "dense_ops.hip")}
    assert notes["bn_nhwc.hip"] == [] and notes["bn_nhwc_core.h"] == ["bn_kernel_name(sel.kernel)"] * 2
    assert [n for n in notes["dense_ops.hip"] if "avgpool" not in n] == ["bn_kernel_name(sel.kernel)"]
    assert [n for n in notes["dense_ops.hip"] if "avgpool" in n] == [f'"avgpool2x2_{k}kernel<{v}>"' for k in ("", "bwd_") for v in (4, 1)]
    for name in ("bn_nhwc.hip", "bn_nhwc_core.h", "dense_ops.hip"):
        src = code(name)
        assert not re.search(r'KD_NOTE_PLUMBING\(\s*"bn_', src), name
        assert "vec4_ok" not in src and "grid_for" not in src and "aligned16" not in src, f"{name}: the launchers decide nothing themselves"
