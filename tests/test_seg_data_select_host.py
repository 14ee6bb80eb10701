"""csrc/seg_data_select.h compiled for the host (tests/seg_data_select_host): the selection the library really runs for kd_seg_crop,
kd_seg_jitter and kd_seg_finish, held to a restated selection on both sides of every gate -- pointer alignment of each operand that
gates, S % 16, S * S % 16, the row length in elements per dtype and layout, W even, W % 32, blur -- plus the constants, the names, the
grids, the argument predicates, and that the header is plain host code whose names the launchers note."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "seg_data_select_host")
CSRC = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
CONSTS = ("TPB", "TX", "TY", "CH", "HDR", "TAPS", "ENTRY", "CAP_C", "CAP_R", "MAX_RADIUS", "JITTER_PIXELS", "VEC_BYTES", "MAX_SIDE", "MAX_BATCH",
          "NCHW", "NHWC", "SK_CROP_1", "SK_JITTER_1", "SK_FINISH_0")
BASE = 0x10000
F32, BF16, NCHW, NHWC = 0, 1, 0, 1


@pytest.fixture(scope="module")
def sel():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libseg_data_select.so"))
    so.ss_name.restype = C.c_char_p
    so.ss_const.restype = so.ss_row_words.restype = so.ss_jitter_workspace.restype = C.c_longlong
    so.ss_crop.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_double)]
    so.ss_jitter.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_double)]
    so.ss_finish.argtypes = [C.c_int] * 3 + [C.c_longlong] * 4 + [C.c_int] * 4 + [C.POINTER(C.c_double)]
    return so


def _call(fn, fields, *args):
    o = (C.c_double * len(fields))()
    fn(*args, o)
    return {k: int(v) for k, v in zip(fields, o)}


def crop(so, S, B=3, img=0, mask=0):
    s = _call(so.ss_crop, ("kernel", "store", "gx", "gy", "gz"), BASE + img, BASE + mask, B, S)
    return dict(s, name=so.ss_name(s["kernel"]).decode())


def jitter(so, S, B=3, img=0):
    s = _call(so.ss_jitter, ("kernel", "pixels", "chunks", "gx", "gy"), BASE + img, B, S)
    return dict(s, name=so.ss_name(s["kernel"]).decode())


def finish(so, dtype, layout, blur, H, W, ld=3, B=3, img=0, mask=0, out=0, mask_out=0):
    s = _call(so.ss_finish, ("kernel", "vec", "src_vec", "gx", "gy", "gz"), dtype, layout, blur, BASE + img, BASE + mask, BASE + out, BASE + mask_out,
              B, H, W, ld)
    return dict(s, name=so.ss_name(s["kernel"]).decode())


def test_constants_and_names(sel):
    K = {n: sel.ss_const(i) for i, n in enumerate(CONSTS)}
    assert (K["TPB"], K["TX"], K["TY"], K["CH"], K["HDR"], K["TAPS"], K["ENTRY"]) == (256, 32, 16, 3, 32, 9, 11)
    assert (K["CAP_C"], K["CAP_R"], K["MAX_RADIUS"], K["JITTER_PIXELS"], K["VEC_BYTES"]) == (74, 42, 5, 16, 16)
    assert (K["NCHW"], K["NHWC"]) == (0, 1) and sel.ss_const(len(CONSTS)) == -1
    assert K["CAP_C"] >= 2 * (K["TX"] - 1) + 1 + K["TAPS"] and K["CAP_R"] >= 2 * (K["TY"] - 1) + 1 + K["TAPS"], "a tile at scale 0.5 fits"
    names = [sel.ss_name(k).decode() for k in range(sel.ss_count())]
    assert sel.ss_count() == 20 and len(set(names)) == 20 and sel.ss_name(20) is None and sel.ss_name(-1) is None
    assert names[:4] == ["seg_crop_kernel<1>", "seg_crop_kernel<16>", "seg_jitter_kernel<1>", "seg_jitter_kernel<16>"]
    k = K["SK_FINISH_0"]
    for d, dn, v in ((0, "f32", 4), (1, "bf16", 8)):
        for l, ln in ((0, "nchw"), (1, "nhwc")):
            for b, bn in ((0, "gather"), (1, "blur")):
                assert names[k + 8 * d + 4 * l + 2 * b] == f"seg_finish_kernel<{dn},{ln},{bn},1>"
                assert names[k + 8 * d + 4 * l + 2 * b + 1] == f"seg_finish_kernel<{dn},{ln},{bn},{v}>"
    assert sel.ss_row_words(24) == 32 + 24 * 24 and sel.ss_row_words(512) == 32 + 24 * 512
    assert sel.ss_jitter_workspace(4) == 32 and sel.ss_jitter_workspace(0) == 0


def test_the_crop_takes_16_byte_stores_only_for_aligned_outputs_and_s_a_multiple_of_16(sel):
    assert crop(sel, 32)["name"] == "seg_crop_kernel<16>" and crop(sel, 32)["store"] == 16
    assert crop(sel, 16)["store"] == 16 and crop(sel, 24)["store"] == 1 and crop(sel, 17)["name"] == "seg_crop_kernel<1>"
    assert crop(sel, 32, img=8)["store"] == 1 and crop(sel, 32, mask=4)["store"] == 1 and crop(sel, 32, img=16, mask=32)["store"] == 16
    for S, gx, gy in ((24, 1, 2), (32, 1, 2), (33, 2, 3), (512, 16, 32), (1, 1, 1)):
        s = crop(sel, S, B=5)
        assert (s["gx"], s["gy"], s["gz"]) == (gx, gy, 5)


def test_the_jitter_owns_16_pixels_a_thread_only_when_a_sample_is_whole_chunks(sel):
    assert jitter(sel, 24) == dict(kernel=3, pixels=16, chunks=36, gx=1, gy=3, name="seg_jitter_kernel<16>")
    assert jitter(sel, 24, img=4)["pixels"] == 1 and jitter(sel, 24, img=4)["chunks"] == 576 and jitter(sel, 24, img=4)["gx"] == 3
    assert jitter(sel, 6)["pixels"] == 1, "36 pixels: not a multiple of 16"
    assert jitter(sel, 4)["pixels"] == 16 and jitter(sel, 4)["chunks"] == 1
    s = jitter(sel, 512, B=4)
    assert (s["chunks"], s["gx"], s["gy"]) == (16384, 64, 4)
    assert jitter(sel, 256)["gx"] == 16 and jitter(sel, 260)["gx"] == 17, "the grid covers the chunks exactly"


@pytest.mark.parametrize("dtype,v", [(F32, 4), (BF16, 8)])
def test_the_finish_stores_gate_on_alignment_row_length_and_even_width(sel, dtype, v):
    for blur in (0, 1):
        assert finish(sel, dtype, NCHW, blur, 24, 24)["vec"] == v
        assert finish(sel, dtype, NCHW, blur, 24, 24, out=v)["vec"] == 1 and finish(sel, dtype, NCHW, blur, 24, 24, mask_out=8)["vec"] == 1
        assert finish(sel, dtype, NCHW, blur, 24, 24, img=1, mask=1)["vec"] == v, "the sources do not gate the stores"
        assert finish(sel, dtype, NCHW, blur, 24, 24 + v // 2)["vec"] == 1, "a row of W elements that is not whole pieces"
        assert finish(sel, dtype, NHWC, blur, 24, 24, ld=3)["vec"] == v and finish(sel, dtype, NHWC, blur, 24, 24, ld=8)["vec"] == v
        assert finish(sel, dtype, NHWC, blur, 40, 44, ld=3)["vec"] == (4 if dtype == F32 else 1), "44 * 3 = 132 elements"
        assert finish(sel, dtype, NHWC, blur, 40, 5, ld=8)["vec"] == 1, "whole pieces but W odd: the mask stores two labels at once"
        assert finish(sel, dtype, NHWC, blur, 40, 6, ld=4)["vec"] == (4 if dtype == F32 else v)
        s = finish(sel, dtype, NHWC, blur, 40, 72, ld=5, B=2)
        assert (s["gx"], s["gy"], s["gz"]) == (3, 3, 2)
        k = finish(sel, dtype, NHWC, blur, 24, 24)["kernel"] - sel.ss_const(CONSTS.index("SK_FINISH_0"))
        assert k == 8 * dtype + 4 + 2 * blur + 1


def test_the_gather_reads_16_bytes_only_from_aligned_sources_of_whole_tiles_and_never_under_the_blur(sel):
    assert finish(sel, F32, NCHW, 0, 1024, 2048)["src_vec"] == 1 and finish(sel, BF16, NHWC, 0, 64, 64, ld=8)["src_vec"] == 1
    assert finish(sel, F32, NCHW, 0, 40, 72)["src_vec"] == 0 and finish(sel, F32, NCHW, 0, 24, 24)["src_vec"] == 0
    assert finish(sel, F32, NCHW, 0, 64, 64, img=4)["src_vec"] == 0 and finish(sel, F32, NCHW, 0, 64, 64, mask=8)["src_vec"] == 0
    assert finish(sel, F32, NCHW, 0, 64, 64, out=4)["src_vec"] == 1, "the outputs do not gate the loads"
    assert finish(sel, F32, NCHW, 1, 64, 64)["src_vec"] == 0 and "blur" in finish(sel, F32, NCHW, 1, 64, 64)["name"]


def test_the_argument_predicates_on_both_sides(sel):
    assert sel.ss_dtype_ok(0) and sel.ss_dtype_ok(1) and not sel.ss_dtype_ok(2) and not sel.ss_dtype_ok(-1)
    assert sel.ss_layout_ok(0) and sel.ss_layout_ok(1) and not sel.ss_layout_ok(2)
    top, bmax = sel.ss_const(CONSTS.index("MAX_SIDE")), sel.ss_const(CONSTS.index("MAX_BATCH"))
    assert sel.ss_side_ok(1) and sel.ss_side_ok(top) and not sel.ss_side_ok(0) and not sel.ss_side_ok(top + 1)
    assert sel.ss_batch_ok(1) and sel.ss_batch_ok(bmax) and not sel.ss_batch_ok(0) and not sel.ss_batch_ok(bmax + 1)


def test_the_selection_header_is_plain_host_code_and_the_launchers_note_its_names():
    with open(os.path.join(CSRC, "seg_data_select.h")) as f:
        hdr = f.read()
    code = re.sub(r"//.*", "", hdr)
    assert "hip" not in code.lower() and "getenv" not in code
    with open(os.path.join(CSRC, "seg_data_ops.hip")) as f:
        src = f.read()
    assert src.count("KD_NOTE_PLUMBING(seg_kernel_name(sel.kernel))") == 3
    assert src.count("seg_crop_select(") == 1 and src.count("seg_jitter_select(") == 1 and src.count("seg_finish_select(") == 1
    assert "& 15" not in src and "aligned16" not in src, "the launchers decide nothing themselves"


def test_the_sweep_program_builds_and_runs_clean():
    """tests/seg_data_select_host/sweep_main.cpp, a program of its own, without the sanitizers (`make sweep` adds them)."""
    subprocess.check_call(["make", "-s", "-C", WRAP, "_build/sweep_plain"])
    out = subprocess.run([os.path.join(WRAP, "_build", "sweep_plain")], capture_output=True, text=True)
    assert out.returncode == 0 and "no finding" in out.stdout, out.stderr
