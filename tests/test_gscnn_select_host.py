"""The shape-stream selection the library really runs (csrc/gscnn_select.h: one selector per entry point of gscnn_ops.hip and
gscnn_bwd.hip, the grids, thread counts, dynamic LDS, the two workspaces), compiled for the host and held against
tests/_shape_stream_cases.py -- without a GPU.  The kernel of every row of the GPU test's case table on the views
test_shape_stream_gpu.py and _shape_stream_child.py build for it; both sides of every gate; every launch figure against the
formulas the launchers had inline before the header existed (PARENT_*, transcribed from them) over sizes that cross every cap and
rounding step; S.sw_blocks / S.sw_workspace against the compiled rule; the name table and the sources' hygiene; the sanitizer
sweep."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import _shape_stream_cases as S

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "gscnn_select_host")
CSRC = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
SOURCES = ("gscnn_ops.hip", "gscnn_bwd.hip")
FIELDS = ("kernel", "why", "grid", "grid2", "threads", "lds", "raise_lds", "sw_blocks", "sw_per_block", "nsx", "nsy", "total", "ws0", "ws1", "ws2",
          "sh", "sw")
CONSTS = ("SL_MAXC", "SW_CH", "SW_PIX_PER_BLOCK", "SW_MAX_BLOCKS", "SC_SEG", "SC_ROWS", "SC_RING", "SC_THREADS_64", "THREADS", "SC_LDS_LIMIT", "GC_PIX",
          "GC_PIX_WIDE", "GC_WIDE_C", "MFMA_PIX", "MFMA_WAVES", "CANNY_GRAD_BYTES", "CANNY_MAG_BYTES", "CANNY_STATE_BYTES", "CANNY_SLACK", "CAP_GATED_MFMA",
          "CAP_POINTWISE_SMALL", "CAP_GATED", "CAP_EDGE_ATTENTION", "CAP_EDGE_ASPP", "CAP_CANNY", "CAP_SMALL_LINEAR", "CAP_GATE_MIX_BWD",
          "CAP_EDGE_ATTENTION_BWD", "CAP_RANK1_ADD")
WHY = ("none", "shape", "dtype", "mask", "channels", "align", "res", "too_large")
DTS = ("f32", "bf16")
ES = {"f32": 4, "bf16": 2}
BASE, BASE2 = 0x10000, 0x4000000     # two buffers' bases (the allocator's are 256-B aligned)
REFUSED = "(refused)"
i32, i64, u64, out = C.c_int, C.c_longlong, C.c_ulonglong, C.POINTER(C.c_double)
SIGS = {"gated_conv": [i32, i64, i32, i64, i32, i64, i32, i32], "edge_attention": [i32, i64, i32, i64], "edge_aspp": [i32, i64, i64, i64, i64] + [i32] * 7,
        "canny": [i32] * 4, "canny_continue": [i32] * 4, "conv3x3_small": [i64, i32, i64, i64, i32, i64, i32] + [i32] * 4,
        "pointwise_small": [i64, i32, i64, i32, i64, i32, i32], "small_linear": [i32] * 6 + [i64, i64, i32], "small_wgrad": [i32] * 6 + [i64],
        "gate_mix_bwd": [i32, i32, i64], "edge_attention_bwd": [i32, i32, i64], "rank1_add": [i32, i64, i32, i64, i32, i64]}


def load():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libgscnn_select.so"))
    so.gs_name.restype = C.c_char_p
    so.gs_const.restype = i64
    so.gs_grid_of.restype, so.gs_grid_of.argtypes = C.c_uint, [i64, i32]
    so.gs_sw_blocks.argtypes = [i64, C.POINTER(i64)]
    so.gs_ws_canny.restype, so.gs_ws_canny.argtypes = u64, [i32] * 3
    so.gs_ws_small_wgrad.restype, so.gs_ws_small_wgrad.argtypes = u64, [i32, i32, i64]
    for name, args in SIGS.items():
        getattr(so, "gs_sel_" + name).argtypes = args + [out]
    return so


@pytest.fixture(scope="module")
def lib():
    return load()


def consts(lib):
    return {n: lib.gs_const(i) for i, n in enumerate(CONSTS)}


def sl_templates(lib):
    return tuple(itertools.takewhile(lambda t: t > 0, (lib.gs_sl_template(i) for i in itertools.count())))


def sw_rule(lib, npix):
    """gs_small_wgrad_blocks -> (blocks, pixels per block)"""
    pb = i64()
    return lib.gs_sw_blocks(npix, C.byref(pb)), pb.value


def call(lib, fn, *args):
    o = (C.c_double * len(FIELDS))()
    getattr(lib, "gs_sel_" + fn)(*args, o)
    sel = dict(zip(FIELDS, o))
    for k in FIELDS[:15]:
        sel[k] = int(sel[k])
    sel["name"] = REFUSED if sel["kernel"] == lib.gs_refused() else lib.gs_name(sel["kernel"]).decode()
    sel["why"] = WHY[sel["why"]]
    return sel


def select(lib, c, mfma=True, dense=True):
    """The selector of the row's entry point on the shape, dtypes and views test_shape_stream_gpu.py (test_gscnn_gpu.py for the
    conv3x3_small rows: dense, or its 80-channel buffers) hands the library for the row."""
    op = c["op"]
    d = lambda k="dt": DTS.index(c[k])
    if op == "small_linear":
        ci, co = c["cin"], c["cout"]
        ydt, ldy = (DTS.index(c["acc"]), co + 16) if c["acc"] else (0, co)
        return call(lib, "small_linear", d("x_dt"), ci + 16 if c["x_slice"] else ci, ci, ydt, ldy, co, S.SL_PIX, BASE if c["mask"] else 0,
                    co + 16 if c["mask"] else 0)
    if op == "small_wgrad":
        pad = 16 if c["sliced"] else 0
        return call(lib, "small_wgrad", d("a_dt"), c["ca"] + pad, c["ca"], d("b_dt"), c["cb"] + pad, c["cb"], c["npix"])
    if op == "gate_mix_bwd":
        return call(lib, "gate_mix_bwd", d(), c["C"], int(np.prod(c["shape"])))
    if op == "edge_attention":
        return call(lib, "edge_attention", d(), BASE, 64, c["npix"])
    if op == "edge_attention_bwd":
        return call(lib, "edge_attention_bwd", d(), 64, c["npix"])
    if op == "edge_aspp":
        return call(lib, "edge_aspp", d(), BASE, BASE, BASE, BASE2 + 16 * ES[c["dt"]], c["C"] + 32, c["N"], *c["hin"], *c["hout"], c["C"])
    if op == "rank1_add":
        y = (BASE2 + 8 * ES[c["dt"]], c["C"] + 16) if c["sliced"] else (BASE2, c["C"])
        return call(lib, "rank1_add", d(), *y, BASE, c["C"], int(np.prod(S.R1_SHAPE)))
    if op == "gated_conv":
        from _shape_stream_child import GC_FEAT_LD, GC_OUT_OFF, GC_OUT_PAD
        return call(lib, "gated_conv", d(), BASE, GC_FEAT_LD, BASE2 + GC_OUT_OFF * ES[c["dt"]], c["C"] + GC_OUT_PAD, c["npix"], c["C"], int(mfma))
    if op == "pointwise_small":
        return call(lib, "pointwise_small", BASE, c["cin"] + 16, BASE2 + S.PW_OUT_OFF * 2, c["cout"] + S.PW_OUT_PAD, c["npix"], c["cin"], c["cout"])
    if op == "canny":
        N, H, W = S.expected_shapes(c)["edges"]
        return call(lib, "canny", N, H, W, 8)
    assert op == "conv3x3_small"
    N, H, W = c["shape"]
    if dense:
        return call(lib, "conv3x3_small", BASE, c["C"], BASE, 0, 0, BASE2, c["C"], N, H, W, c["C"])
    return call(lib, "conv3x3_small", BASE, S.C3_LD, BASE, BASE2 + 8 * 2, S.C3_LD, BASE2 + 0x1000000, S.C3_LD, N, H, W, c["C"])


# ---- the case table ------------------------------------------------------------------------------------------------------------------
ROWS = S.CASES + S.C3_ROWS


@pytest.mark.parametrize("c", ROWS, ids=S.ids(ROWS))
def test_every_row_selects_its_kernel(lib, c):
    sel = select(lib, c)
    assert sel["name"] == S.slot_name(c), f"{c['id']}: gscnn_select.h picks {sel['name']}, the row says {S.slot_name(c)}"
    assert sel["why"] == "none" and sel["grid"] >= 1 and sel["grid2"] >= 1
    if c["op"] == "conv3x3_small":
        assert select(lib, c, dense=False) == sel
    if c["op"] == "canny":
        N, H, W = S.expected_shapes(c)["edges"]
        assert call(lib, "canny_continue", N, H, W, 8)["name"] == c["then"]
    if c in S.GC_VALU_BF16:
        assert select(lib, c, mfma=False)["name"] == S.slot_name(c, mfma=False) == f"gated_conv_kernel<bf16,{c['C']}>"


def test_the_names_are_distinct_and_every_one_has_a_row(lib):
    n = lib.gs_refused()
    names = [lib.gs_name(k).decode() for k in range(n)]
    assert lib.gs_name(n) is None and lib.gs_name(-1) is None
    assert len(set(names)) == n == 31
    named = {S.slot_name(c) for c in ROWS} | {c["then"] for c in S.cases_of("canny")} | {S.slot_name(c, mfma=False) for c in S.GC_VALU_BF16}
    assert named == set(names), sorted(named ^ set(names))


# ---- the launch figures of the launchers before the header: kernel, grid(s), threads, dynamic LDS ------------------------------------
def parent_blocks_for(total, cap):
    b = (total + 255) // 256
    return 1 if b < 1 else min(b, cap)


def parent_gated_conv(dt, npix, Cc, mfma):
    if mfma and dt == "bf16":
        waves = (npix + 15) // 16
        return f"gated_conv_mfma_kernel<{Cc}>", parent_blocks_for((waves + 3) // 4 * 256, 256 * 32)
    return f"gated_conv_kernel<{dt},{Cc}>", parent_blocks_for((npix + (1 if Cc >= 32 else 3)) // (2 if Cc >= 32 else 4), 65536)


def parent_small_linear(cout):
    return "small_linear_kernel<%d>" % (8 if cout <= 8 else 16 if cout <= 16 else 24 if cout <= 24 else 40 if cout <= 40 else 72)


def parent_sw_blocks(npix):
    nb = (npix + 4095) // 4096
    if nb > 1024:
        nb = 1024
    if nb < 1:
        nb = 1
    pb = (npix + nb - 1) // nb
    pb = (pb + 64 - 1) // 64 * 64
    return (npix + pb - 1) // pb, pb


def parent_sw_workspace(ca, cb, npix):
    return 0 if ca < 1 or cb < 1 or npix < 1 else parent_sw_blocks(npix)[0] * (ca * cb + cb) * 4


def parent_canny_workspace(N, H, W):
    return N * H * W * (4 + 4 + 1) + 256


def parent_conv3x3(N, H, W, Cc):
    nsx, nsy = (W + 255) // 256, (H + 15) // 16
    return dict(name=f"conv3x3_small_kernel<{Cc}>", nsx=nsx, nsy=nsy, grid=N * nsx * nsy, threads=512 if Cc == 64 else 256,
                lds=4 * (256 + 2) * (Cc * 2 + 16 if Cc == 64 else Cc * 2), raise_lds=int(Cc in (64, 32)))


def around(cap, per_thread=1):
    """Item counts around the size at which `cap` workgroups of 256 threads of `per_thread` items each stop covering the work, and
    around the rounding steps below it."""
    edge = cap * 256 * per_thread
    near = sorted({edge + s * k + e for s in (-1, 1) for k in (0, 1, per_thread, 256 * per_thread) for e in (-1, 0, 1)})
    return [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537] + [n for n in near if n > 0] + [2 * edge, 2 ** 31 - 1, 2 ** 31, 2 ** 40]


def test_grids_threads_and_lds_are_the_parents(lib):
    K = consts(lib)
    assert (K["CAP_GATED_MFMA"], K["CAP_POINTWISE_SMALL"], K["CAP_GATED"], K["CAP_EDGE_ATTENTION"], K["CAP_EDGE_ASPP"], K["CAP_CANNY"]) == (8192, 8192, 65536, 65536, 65536, 65536)
    assert (K["CAP_SMALL_LINEAR"], K["CAP_GATE_MIX_BWD"], K["CAP_EDGE_ATTENTION_BWD"], K["CAP_RANK1_ADD"]) == (1 << 16, 1 << 16, 1 << 16, 1 << 20)
    seen = set()
    for dt, Cc, mfma in itertools.product(DTS, (8, 16, 32), (0, 1)):
        matrix = mfma and dt == "bf16"
        for npix in around(8192, 64) if matrix else around(65536, 2 if Cc == 32 else 4):
            sel = call(lib, "gated_conv", DTS.index(dt), BASE, 64, BASE2, Cc, npix, Cc, mfma)
            assert (sel["name"], sel["grid"]) == parent_gated_conv(dt, npix, Cc, mfma) and (sel["threads"], sel["lds"], sel["raise_lds"]) == (256, 0, 0)
            seen.add((sel["name"], sel["grid"] == (8192 if matrix else 65536)))
    assert {s[1] for s in seen if "mfma" in s[0]} == {s[1] for s in seen if "mfma" not in s[0]} == {True, False}
    for npix in around(65536):
        for dt in DTS:
            sel = call(lib, "edge_attention", DTS.index(dt), BASE, 8, npix)
            assert (sel["name"], sel["grid"], sel["threads"], sel["lds"]) == (f"edge_attention_kernel<{dt}>", parent_blocks_for(npix, 65536), 256, 0)
        for fn, args in (("small_linear", (0, 8, 8, 0, 8, 8, npix, 0, 0)), ("gate_mix_bwd", (0, 8, npix)), ("edge_attention_bwd", (0, 8, npix))):
            sel = call(lib, fn, *args)
            assert (sel["grid"], sel["threads"], sel["lds"]) == (parent_blocks_for(npix, 1 << 16), 256, 0), (fn, npix)
    for npix in around(8192, 64):
        for ci, co in ((64, 32), (32, 16), (16, 8)):
            sel = call(lib, "pointwise_small", BASE, ci, BASE2, co, npix, ci, co)
            waves = (npix + 15) // 16
            assert (sel["name"], sel["grid"], sel["threads"], sel["lds"]) == (f"pointwise_small_kernel<{ci},{co}>", parent_blocks_for((waves + 3) // 4 * 256, 256 * 32), 256, 0)
    for Cc in (8, 64):
        for items in around(1 << 20):                      # a thread owns 8 channels of a pixel
            npix = -(-items // (Cc // 8))
            for dt in DTS:
                sel = call(lib, "rank1_add", DTS.index(dt), BASE, Cc, BASE2, Cc, npix)
                assert (sel["name"], sel["grid"], sel["threads"]) == (f"rank1_add_kernel<{dt}>", parent_blocks_for(npix * (Cc // 8), 1 << 20), 256)
    f = np.float32
    for N, (H, W), (Ho, Wo), Cc in itertools.product((1, 2, 5), ((1, 8), (7, 1), (10, 14), (1024, 2048)), ((1, 1), (4, 6), (9, 13), (129, 257), (1024, 2048)), (8, 16, 256)):
        for dt in DTS:
            sel = call(lib, "edge_aspp", DTS.index(dt), BASE, BASE, BASE, BASE2, Cc, N, H, W, Ho, Wo, Cc)
            assert (sel["name"], sel["grid"], sel["threads"]) == (f"edge_aspp_kernel<{dt}>", parent_blocks_for(N * Ho * Wo * (Cc // 8), 65536), 256)
            want = [f(H - 1) / f(Ho - 1) if Ho > 1 else f(0), f(W - 1) / f(Wo - 1) if Wo > 1 else f(0)]
            assert np.array([sel["sh"], sel["sw"]], dtype=f).tobytes() == np.array(want, dtype=f).tobytes()
    assert call(lib, "edge_aspp", 0, BASE, BASE, BASE, BASE2, 8, 1, 4, 4, 4096, 4096, 8)["grid"] == 65536       # 2^24 items: exactly the cap
    assert call(lib, "edge_aspp", 0, BASE, BASE, BASE, BASE2, 8, 1, 4, 4, 4095, 4096, 8)["grid"] == 65520
    for N, H, W in itertools.product((1, 2, 3), (1, 9, 255, 256, 257, 4096), (1, 7, 1400, 4096, 65536)):
        n = N * H * W
        assert lib.gs_ws_canny(N, H, W) == parent_canny_workspace(N, H, W)
        for fn, name in (("canny", "canny_grad_kernel"), ("canny_continue", "canny_hyst_kernel")):
            sel = call(lib, fn, N, H, W, 8)
            assert (sel["name"], sel["grid"], sel["threads"], sel["total"]) == (name, parent_blocks_for(n, 65536), 256, n)
            assert (sel["ws0"], sel["ws1"], sel["ws2"]) == (0, 4 * n, 8 * n) and sel["ws2"] + n <= lib.gs_ws_canny(N, H, W)
    for N, H, W, Cc in itertools.product((1, 2, 8), (1, 15, 16, 17, 33, 1024), (1, 255, 256, 257, 513, 2048), (16, 32, 64)):
        sel = call(lib, "conv3x3_small", BASE, Cc, BASE, 0, 0, BASE2, Cc, N, H, W, Cc)
        want = parent_conv3x3(N, H, W, Cc)
        assert {k: sel[k] for k in want} == want
    assert [sel["lds"] for sel in (call(lib, "conv3x3_small", BASE, Cc, BASE, 0, 0, BASE2, Cc, 1, 1, 1, Cc) for Cc in (16, 32, 64))] == [33024, 66048, 148608]


def test_small_wgrad_plan_and_workspace_are_the_parents_and_the_tables(lib):
    K = consts(lib)
    assert (K["SW_CH"], K["SW_PIX_PER_BLOCK"], K["SW_MAX_BLOCKS"]) == (S.SW_CH, S.SW_PIX_PER_BLOCK, S.SW_MAX_BLOCKS) == (64, 4096, 1024)
    sizes = sorted(set(S.SW_NPIX + S.SW_PLAN_ONLY_NPIX + [c["npix"] for c in S.cases_of("small_wgrad")] + [2, 127, 128, 129, 4095, 8191, 8192, 8193]
                       + [4096 * k + e for k in (2, 3, 1023, 1024, 1025, 4096) for e in (-65, -64, -1, 0, 1, 63, 64, 65)] + [2 ** 31 - 1, 2 ** 31, 2 ** 40 + 77]))
    for npix in sizes:
        assert sw_rule(lib, npix) == parent_sw_blocks(npix) == S.sw_blocks(npix), npix
        for ca, cb in S.SW_PAIRS + [(33, 72)]:
            sel = call(lib, "small_wgrad", 0, ca, ca, 1, cb, cb, npix)
            nb, pb = parent_sw_blocks(npix)
            assert (sel["name"], sel["grid"], sel["sw_blocks"], sel["sw_per_block"], sel["grid2"], sel["threads"], sel["lds"]) == \
                ("small_wgrad_partial_kernel", nb, nb, pb, (ca * cb + cb + 255) // 256, 256, 0)
            assert lib.gs_ws_small_wgrad(ca, cb, npix) == parent_sw_workspace(ca, cb, npix) == S.sw_workspace(ca, cb, npix)
    assert [lib.gs_ws_small_wgrad(*a) for a in ((0, 8, 100), (8, 0, 100), (8, 8, 0), (-1, 8, 100), (8, 8, -5))] == [0] * 5
    assert any(sw_rule(lib, n)[0] == 1024 for n in S.SW_PLAN_ONLY_NPIX) and any(sw_rule(lib, n)[0] < 1024 for n in S.SW_PLAN_ONLY_NPIX)


def test_gs_grid_at_every_call_sites_cap(lib):
    K = consts(lib)
    for name in CONSTS[19:]:
        cap = K[name]
        assert [lib.gs_grid_of(cap * 256 + d, cap) for d in (-256, -255, -1, 0, 1)] == [cap - 1, cap, cap, cap, cap], name
        assert [lib.gs_grid_of(t, cap) for t in (-5, 0, 1, 256, 257, 2 ** 62)] == [1, 1, 1, 1, 2, cap]
        for t in around(cap):
            assert lib.gs_grid_of(t, cap) == parent_blocks_for(t, cap)
    assert [lib.gs_dtype_is_ok(d) for d in (-1, 0, 1, 2)] == [0, 1, 1, 0]


# ---- both sides of every gate -------------------------------------------------------------------------------------------------------
def test_small_linear_template_boundaries_and_the_channel_limit(lib):
    K, templates = consts(lib), sl_templates(lib)
    assert templates == S.SL_TEMPLATES == (8, 16, 24, 40, 72) and K["SL_MAXC"] == S.SL_MAXC == templates[-1]
    sl = lambda ci, co, ldx=None, ldy=None, xdt=0, ydt=0, npix=70, mask=0, ldm=0: call(lib, "small_linear", xdt, ldx or ci, ci, ydt, ldy or co, co, npix, mask, ldm)
    for co in range(1, 73):
        assert sl(33, co)["name"] == parent_small_linear(co) == f"small_linear_kernel<{S.sl_template(co)}>"
    for t in templates[:-1]:
        assert sl(1, t)["name"] != sl(1, t + 1)["name"]
    for ci, co in ((72, 72), (1, 1)):
        assert sl(ci, co)["why"] == "none"
    for ci, co in S.SL_REFUSED + [(0, 8), (8, 0), (-3, 8)]:
        sel = sl(ci, co, ldx=80, ldy=80)
        assert (sel["name"], sel["why"]) == (REFUSED, "channels"), (ci, co)
    assert sl(33, 8, ldx=32)["why"] == sl(33, 8, ldy=7)["why"] == "channels" and sl(33, 8, ldx=33, ldy=8)["why"] == "none"      # a row shorter than its channels
    assert sl(8, 8, mask=BASE, ldm=7)["why"] == "mask" and sl(8, 8, mask=BASE, ldm=8)["why"] == "none" and sl(8, 8, mask=0, ldm=0)["why"] == "none"
    assert sl(8, 8, xdt=2)["why"] == sl(8, 8, ydt=-1)["why"] == "dtype" and sl(8, 8, xdt=1, ydt=1)["why"] == "none"
    assert sl(8, 8, npix=0)["why"] == sl(8, 8, npix=-1)["why"] == "shape"
    assert sl(73, 8, xdt=2, mask=BASE, ldm=7)["why"] == "dtype" and sl(73, 8, mask=BASE, ldm=7)["why"] == "mask"               # the entry point's order of checks
    sw = lambda ca, cb, lda=None, ldb=None, adt=0, bdt=0, npix=70: call(lib, "small_wgrad", adt, lda or ca, ca, bdt, ldb or cb, cb, npix)
    assert sw(72, 72)["why"] == sw(1, 1)["why"] == "none"
    for ca, cb in ((73, 8), (8, 73), (0, 8), (8, 0)):
        assert sw(ca, cb, lda=80, ldb=80)["why"] == "channels"
    assert sw(33, 8, lda=32)["why"] == sw(33, 8, ldb=7)["why"] == "channels"
    assert sw(8, 8, adt=2)["why"] == sw(8, 8, bdt=2)["why"] == "dtype" and sw(8, 8, npix=0)["why"] == "shape" and sw(73, 8, adt=2)["why"] == "dtype"


def test_gated_conv_gates(lib):
    K = consts(lib)
    assert (K["GC_PIX"], K["GC_PIX_WIDE"], K["GC_WIDE_C"], K["MFMA_PIX"], K["MFMA_WAVES"]) == (4, 2, 32, 16, 4)
    assert [lib.gs_gated_pix_of(c) for c in (8, 16, 32)] == [4, 4, 2]
    gc = lambda dt, Cc, mfma=1, foff=0, ooff=0, ldf=64, ldo=None, npix=546: call(lib, "gated_conv", DTS.index(dt), BASE + foff, ldf, BASE2 + ooff,
                                                                                 ldo or Cc + 16, npix, Cc, mfma)
    for Cc in (8, 16, 32):
        assert gc("bf16", Cc, 1)["name"] == f"gated_conv_mfma_kernel<{Cc}>" and gc("bf16", Cc, 0)["name"] == f"gated_conv_kernel<bf16,{Cc}>"
        assert gc("f32", Cc, 1) == gc("f32", Cc, 0) and gc("f32", Cc)["name"] == f"gated_conv_kernel<f32,{Cc}>"          # the switch means nothing to fp32
    for Cc in (0, 4, 12, 24, 33, 64):
        assert (gc("f32", Cc)["name"], gc("bf16", Cc)["why"]) == (REFUSED, "channels")
    for dt in DTS:
        e = 16 // ES[dt]                                       # elements in 16 bytes
        for mfma in (0, 1):
            assert gc(dt, 16, mfma, foff=ES[dt])["why"] == gc(dt, 16, mfma, ooff=ES[dt])["why"] == "align"                # a base one element off
            assert gc(dt, 16, mfma, foff=8)["why"] == gc(dt, 16, mfma, ooff=8)["why"] == "align"                          # ... 8 bytes off, bf16 on the matrix cores too
            assert gc(dt, 16, mfma, ldf=64 + 1)["why"] == gc(dt, 16, mfma, ldo=32 + 1)["why"] == "align"                  # a leading dimension one element off
            assert gc(dt, 16, mfma, ldf=64 + e // 2)["why"] == gc(dt, 16, mfma, ldo=32 + e // 2)["why"] == "align"        # ... 8 bytes off
            assert gc(dt, 16, mfma, foff=16, ooff=32, ldf=64 + e, ldo=32 + e)["why"] == "none"
    assert gc("f32", 16, npix=0)["why"] == "shape" and call(lib, "gated_conv", 2, BASE, 64, BASE2, 32, 5, 12, 1)["why"] == "dtype"
    assert gc("f32", 12, foff=4)["why"] == "channels"                                                                      # channels before alignment


def test_alignment_and_channel_gates_of_the_other_entry_points(lib):
    for dt in DTS:
        n, es = DTS.index(dt), ES[dt]
        e = 16 // es
        ea = lambda off=0, ld=64, npix=9, d=n: call(lib, "edge_attention", d, BASE + off, ld, npix)
        assert ea()["why"] == ea(off=16, ld=64 + e)["why"] == "none"
        assert ea(off=es)["why"] == ea(ld=65)["why"] == ea(off=8)["why"] == ea(ld=64 + e // 2)["why"] == "align"
        assert ea(npix=0)["why"] == "shape" and ea(d=3)["why"] == "dtype"
        eb = lambda ldc=64, npix=9, d=n: call(lib, "edge_attention_bwd", d, ldc, npix)
        assert eb(8)["why"] == eb(9)["why"] == "none" and eb(7)["why"] == eb(d=2)["why"] == "dtype" and eb(npix=0)["why"] == "shape"
        gm = lambda Cc=8, npix=9, d=n: call(lib, "gate_mix_bwd", d, Cc, npix)
        assert gm(1)["why"] == gm(33)["why"] == "none" and gm(0)["why"] == gm(npix=0)["why"] == "shape" and gm(d=-1)["why"] == "dtype"
        ap = lambda Cc=16, yoff=0, ldy=48, w=BASE, sc=BASE, sf=BASE, shape=(2, 10, 14, 4, 6), d=n: call(lib, "edge_aspp", d, w, sc, sf, BASE2 + yoff, ldy, *shape, Cc)
        assert ap()["why"] == ap(Cc=8, yoff=16, ldy=48 + e)["why"] == "none"
        assert ap(Cc=12)["why"] == ap(yoff=es)["why"] == ap(ldy=49)["why"] == ap(ldy=48 + e // 2)["why"] == "align"
        assert ap(w=BASE + 4)["why"] == ap(sc=BASE + 4)["why"] == ap(sf=BASE + 8)["why"] == "align" and ap(w=BASE + 16)["why"] == "none"
        assert ap(d=2)["why"] == "dtype" and ap(Cc=0)["why"] == "shape"
        for i in range(5):
            shape = [2, 10, 14, 4, 6]
            shape[i] = 0
            assert ap(shape=tuple(shape))["why"] == "shape"
        r1 = lambda Cc=16, yoff=0, ldy=32, woff=0, npix=48, d=n: call(lib, "rank1_add", d, BASE2 + yoff, ldy, BASE + woff, Cc, npix)
        assert r1()["why"] == r1(Cc=8, yoff=16, ldy=32 + e)["why"] == r1(Cc=64, ldy=64)["why"] == "none"
        assert r1(Cc=S.R1_REFUSED_C)["why"] == r1(Cc=4)["why"] == r1(yoff=es)["why"] == r1(ldy=33)["why"] == r1(ldy=32 + e // 2)["why"] == r1(woff=4)["why"] == "align"
        assert r1(Cc=0)["why"] == r1(npix=0)["why"] == "shape" and r1(d=2)["why"] == "dtype"
    # kd_rank1_add as test_shape_stream_gpu.py's refusal calls it: dense fp32, 12 channels
    assert call(lib, "rank1_add", 0, BASE2, S.R1_REFUSED_C, BASE, S.R1_REFUSED_C, 48)["name"] == REFUSED
    pw = lambda ci, co, xoff=0, ldx=None, yoff=0, ldy=None, npix=17: call(lib, "pointwise_small", BASE + xoff, ldx or ci + 16, BASE2 + yoff, ldy or co + 12, npix, ci, co)
    for ci, co in ((64, 32), (32, 16), (16, 8)):
        assert pw(ci, co)["name"] == f"pointwise_small_kernel<{ci},{co}>" and pw(ci, co, ldx=ci, ldy=co, xoff=16, yoff=8)["why"] == "none"
        assert pw(ci, co, xoff=8)["why"] == pw(ci, co, xoff=2)["why"] == pw(ci, co, ldx=ci + 4)["why"] == pw(ci, co, ldx=ci - 8)["why"] == "align"
        assert pw(ci, co, yoff=4)["why"] == pw(ci, co, yoff=2)["why"] == pw(ci, co, ldy=co + 2)["why"] == pw(ci, co, ldy=co - 4)["why"] == "align"
        assert pw(ci, co, npix=0)["why"] == "shape"
    for ci, co in ((64, 16), (32, 32), (16, 16), (8, 4), (128, 64), (32, 8)):
        assert (pw(ci, co)["name"], pw(ci, co)["why"]) == (REFUSED, "channels")
    assert pw(64, 16, xoff=8)["why"] == "channels"
    c3 = lambda Cc=32, xoff=0, ldx=None, woff=0, res=0, ldres=None, yoff=0, ldy=None, shape=(2, 37, 45): call(
        lib, "conv3x3_small", BASE + xoff, ldx or Cc, BASE + 0x100000 + woff, res, ldres or Cc, BASE2 + yoff, ldy or Cc, *shape, Cc)
    for Cc in (16, 32, 64):
        assert c3(Cc)["name"] == c3(Cc, xoff=16, yoff=32, ldx=Cc + 8, ldy=Cc + 16, res=BASE2 + 0x100000, ldres=Cc + 8)["name"] == f"conv3x3_small_kernel<{Cc}>"
        assert c3(Cc, xoff=8)["why"] == c3(Cc, yoff=2)["why"] == c3(Cc, woff=8)["why"] == c3(Cc, ldx=Cc + 4)["why"] == c3(Cc, ldy=Cc + 1)["why"] == "align"
        assert c3(Cc, ldx=Cc - 8)["why"] == c3(Cc, ldy=Cc - 8)["why"] == "align"
        assert c3(Cc, res=BASE + 8)["why"] == c3(Cc, res=BASE, ldres=Cc + 4)["why"] == c3(Cc, res=BASE, ldres=Cc - 8)["why"] == "res"
        assert c3(Cc, res=0, ldres=3)["why"] == "none"                                           # without a residual its stride means nothing
        assert c3(Cc, shape=(0, 3, 3))["why"] == c3(Cc, shape=(1, 0, 3))["why"] == c3(Cc, shape=(1, 3, -1))["why"] == "shape"
    for Cc in (8, 24, 48, 128):
        assert c3(Cc)["why"] == "channels"
    # "image too large": the first workgroup count above a 32-bit grid
    sel = c3(16, shape=(2 ** 31 - 1, 16, 256))
    assert (sel["name"], sel["grid"], sel["nsx"], sel["nsy"]) == ("conv3x3_small_kernel<16>", 2 ** 31 - 1, 1, 1)
    assert c3(16, shape=(2 ** 30, 17, 256))["why"] == "too_large" and (2 ** 30) * 2 == 2 ** 31 > 2 ** 31 - 1
    assert c3(16, shape=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))["why"] == "too_large"             # a count no 64-bit integer holds
    for fn in ("canny", "canny_continue"):
        assert call(lib, fn, 1, 9, 1400, 8)["why"] == "none"
        assert [call(lib, fn, *a, 8)["why"] for a in ((0, 9, 9), (1, 0, 9), (1, 9, 0), (-1, 9, 9))] == ["shape"] * 4 and call(lib, fn, 1, 9, 9, -1)["why"] == "shape"
    assert call(lib, "canny", 1, 9, 9, 0)["why"] == "none" and call(lib, "canny_continue", 1, 9, 9, 0)["why"] == "shape"      # kd_canny may run no sweep


# ---- hygiene ------------------------------------------------------------------------------------------------------------------------
def sources():
    texts = []
    for name in SOURCES:
        with open(os.path.join(CSRC, name)) as f:
            texts.append(f.read())
    return texts


def test_every_note_goes_through_the_table():
    for name, text in zip(SOURCES, sources()):
        assert not re.search(r'KD_NOTE_PLUMBING\(\s*"', text), name
        notes = re.findall(r'KD_NOTE_PLUMBING\(([^;]*)\);', text)
        assert notes and set(notes) == {"gs_kernel_name(sel.kernel)"}, (name, notes)
    assert sum(len(re.findall(r'KD_NOTE_PLUMBING\(', t)) for t in sources()) == len(SIGS)       # once per entry point


def test_the_conv_log_literals_are_the_three_they_were():
    """bench.py, test_bf16_path_gpu.py and _shape_stream_child.py read that log and assert name sets."""
    seen = [n for t in sources() for n in re.findall(r'KD_NOTE_KERNEL\(([^;]*)\);', t)]
    assert sorted(seen) == ['"conv3x3_small_kernel<64>"', '"gated_conv_kernel"', '"gated_conv_mfma_kernel"']


def test_the_environment_is_read_in_one_place():
    assert sum(t.count("getenv") for t in sources()) == 1 and 'getenv("KDCC_GATED_MFMA")' in sources()[0]


def test_the_selection_header_is_plain_host_code():
    with open(os.path.join(CSRC, "gscnn_select.h")) as f:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
    assert not re.search(r"\bhip\w*|\bgetenv\b|__global__|__device__", text, flags=re.I)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", "<stdint.h>", '"../../include/kdcc.h"', '"resample.h"']
    # no state: the only statics are the inline functions and the constant name table
    statics = re.findall(r"^\s*static\s+(?!inline\b|const char \*const names\[\]|_?assert)[^\n]*", re.sub(r"static_assert", "_assert", text), flags=re.M)
    assert not statics, statics


def test_the_sanitizer_sweep_builds_and_finds_nothing():
    r = subprocess.run(["make", "-s", "-C", WRAP, "sweep"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "no finding" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
