"""The bilinear resampling rule every kernel and selector shares (csrc/resample.h), compiled for the host and held against a
float32 numpy restatement written here -- without a GPU.  The geometry and the source rule bit for bit; the source index against
float64 index arithmetic; and the two properties the backward kernels rest on: every output a source index weighs lies inside its
candidate range (cover), and one output's adjoint weights add up to its forward weights (partition).

The header states o * s + off in plain C, so the host build (tests/resample_host/Makefile: -ffp-contract=off) rounds the product
first and the restatement does the same.

Index check: a float64 coordinate within 1e-4 of an integer says nothing about a float32 floor, but leaving all of those out would
leave out 17.0 % (align_corners) and 9.3 % (half-pixel) of this sweep: every o = 0, every I == O, every integer ratio.  Most of them
are computed exactly in float32 (the float32 coordinate equals the float64 one), where the index is not in doubt, so they are
checked too; what stays excluded is a near-integer coordinate that float32 does not hit exactly, 0.44 % of the sweep, held under
5 %."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "resample_host")
HEADER = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc", "resample.h")
f32 = np.float32
PAIRS = list(itertools.product(range(1, 41), range(1, 41))) + [(33, 1025), (128, 1024), (256, 2048), (1025, 33)]     # (I, O)
AXES = [(I, O, ac) for ac in (1, 0) for I, O in PAIRS]
i32, pi, pf = C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libresample.so"))
    so.rs_geom.argtypes = [i32] * 5 + [pf]
    so.rs_src.argtypes = [i32, i32, C.c_float, C.c_float, pi, pi, pf]
    so.rs_src_ac.argtypes = [i32, i32, C.c_float, pi, pi, pf]
    so.rs_weight_ac.argtypes = [i32, i32, C.c_float, pf]
    so.rs_lerp.restype, so.rs_lerp.argtypes = C.c_float, [C.c_float] * 3
    so.rs_range.argtypes = [i32, i32, C.c_float, C.c_float, pi, pi]
    so.rs_weight.argtypes = [i32, i32, C.c_float, C.c_float, pf]
    return so


# ---- the restatement: float32 numpy, one rounding per operation ------------------------------------------------------------------------
def geom(h, w, H, W, align):
    sh = f32(h - 1) / f32(H - 1) if H > 1 else f32(0)
    sw = f32(w - 1) / f32(W - 1) if W > 1 else f32(0)
    oh = ow = f32(0)
    if not align:
        sh, sw = f32(h) / f32(H), f32(w) / f32(W)
        oh, ow = f32(0.5) * sh - f32(0.5), f32(0.5) * sw - f32(0.5)
    return [sh, sw, oh, ow]


def src_rule(I, O, s, off):
    """(i0, i1, f, src) of every output index, unfused: the product is rounded, then the sum."""
    src = np.maximum(np.arange(O).astype(f32) * s + off, f32(0))
    assert src.dtype == f32
    i0 = np.minimum(src.astype(np.int32), I - 1)
    i1 = np.minimum(i0 + 1, I - 1)
    return i0, i1, src - i0.astype(f32), src


def axis_geom(I, O, ac):
    g = geom(I, I, O, O, ac)
    return g[0], g[2]


def got_src(lib, I, O, s, off):
    i0, i1, f = np.empty(O, np.int32), np.empty(O, np.int32), np.empty(O, f32)
    lib.rs_src(I, O, s, off, i0.ctypes.data_as(pi), i1.ctypes.data_as(pi), f.ctypes.data_as(pf))
    return i0, i1, f


@pytest.fixture(scope="module")
def sweep(lib):
    """Every axis of the sweep once, shared by the tests below: the header's (i0, i1, f), ranges and O x I weights."""
    out = {}
    for I, O, ac in AXES:
        s, off = axis_geom(I, O, ac)
        lo, hi, w = np.empty(I, np.int32), np.empty(I, np.int32), np.empty((O, I), f32)
        lib.rs_range(I, O, s, off, lo.ctypes.data_as(pi), hi.ctypes.data_as(pi))
        lib.rs_weight(I, O, s, off, w.ctypes.data_as(pf))
        out[I, O, ac] = (s, off) + got_src(lib, I, O, s, off) + (lo, hi, w)
    return out


# ---- 1. geometry -----------------------------------------------------------------------------------------------------------------------
def test_the_geometry_is_the_restatement_bit_for_bit(lib):
    ext = (1, 2, 3, 5, 7, 33, 128, 1024)
    for h, w, H, W, align in itertools.product(ext, ext, ext, ext, (1, 0)):
        got = (C.c_float * 4)()
        lib.rs_geom(h, w, H, W, align, got)
        assert np.array(got, dtype=f32).tobytes() == np.array(geom(h, w, H, W, align), dtype=f32).tobytes(), (h, w, H, W, align)


# ---- 2. the source rule ------------------------------------------------------------------------------------------------------------------
def test_the_source_rule_is_the_restatement_bit_for_bit_and_stays_inside_the_axis(sweep):
    for (I, O, ac), (s, off, i0, i1, f, *_) in sweep.items():
        w0, w1, wf, _ = src_rule(I, O, s, off)
        assert np.array_equal(i0, w0) and np.array_equal(i1, w1) and f.tobytes() == wf.tobytes(), (I, O, ac)
        assert (0 <= i0).all() and (i0 <= i1).all() and (i1 <= I - 1).all() and (i1 - i0 <= 1).all(), (I, O, ac)
        # the parent's rule gives f < 1 everywhere, the clamped last index included: no coordinate of these geometries reaches I
        assert (f >= 0).all() and (f < 1).all(), (I, O, ac)


def test_the_align_corners_form_without_an_offset_is_the_rule_at_offset_zero(lib, sweep):
    for (I, O, ac), (s, off, i0, i1, f, lo, hi, w) in sweep.items():
        if ac:
            g0, g1, gf, gw = np.empty(O, np.int32), np.empty(O, np.int32), np.empty(O, f32), np.empty((O, I), f32)
            lib.rs_src_ac(I, O, s, g0.ctypes.data_as(pi), g1.ctypes.data_as(pi), gf.ctypes.data_as(pf))
            lib.rs_weight_ac(I, O, s, gw.ctypes.data_as(pf))
            assert off == 0 and np.array_equal(g0, i0) and np.array_equal(g1, i1) and gf.tobytes() == f.tobytes(), (I, O)
            assert gw.tobytes() == w.tobytes(), (I, O)


def test_the_source_index_is_float64_interpolate_index_arithmetic(sweep):
    total = near_int = excluded = 0
    for (I, O, ac), (s, off, i0, *_) in sweep.items():
        o = np.arange(O, dtype=np.float64)
        src = o * ((I - 1) / (O - 1) if O > 1 else 0.0) if ac else np.maximum((o + 0.5) * I / O - 0.5, 0.0)
        near = np.abs(src - np.round(src)) < 1e-4
        skip = near & (src_rule(I, O, s, off)[3].astype(np.float64) != src)
        want = np.minimum(np.floor(src).astype(np.int64), I - 1)
        assert np.array_equal(i0[~skip], want[~skip]), (I, O, ac)
        total, near_int, excluded = total + O, near_int + int(near.sum()), excluded + int(skip.sum())
    print(f"(I, O, o) triples: {total}; within 1e-4 of an integer: {near_int / total:.4%}; of those not exact in float32, excluded: {excluded / total:.4%}")
    assert excluded / total < 0.05


def test_lerp_operand_order(lib):
    r = np.random.default_rng(0)
    for fr, a, b in r.standard_normal((200, 3)).astype(f32):
        fr = f32(abs(fr) % 1)
        assert f32(lib.rs_lerp(fr, a, b)).tobytes() == ((f32(1) - fr) * a + fr * b).tobytes()


# ---- 3. cover: what the backward kernels rest on ---------------------------------------------------------------------------------------
def test_every_weighed_output_lies_in_the_candidate_range(sweep):
    for (I, O, ac), (s, off, i0, i1, f, lo, hi, w) in sweep.items():
        assert (0 <= lo).all() and (hi <= O - 1).all(), (I, O, ac)
        if s > 0:
            assert (hi - lo <= 2.0 / float(s) + 6).all(), (I, O, ac, int((hi - lo).max()))
        o = np.arange(O)[:, None]
        assert not (w != 0)[(o < lo[None, :]) | (o > hi[None, :])].any(), (I, O, ac)


# ---- 4. partition: the adjoint uses the forward's weights --------------------------------------------------------------------------------
def test_the_adjoint_weights_of_an_output_are_its_forward_weights(sweep):
    for (I, O, ac), (s, off, i0, i1, f, lo, hi, w) in sweep.items():
        want = np.zeros((O, I), f32)
        rows = np.arange(O)
        want[rows, i0] += f32(1) - f
        want[rows, i1] += f          # i0 == i1 (the clamped end): one entry holds (1 - f) + f
        assert w.tobytes() == want.tobytes(), (I, O, ac)
        acc = np.zeros(O, f32)
        for i in range(I):           # the sum over i in index order, in float32
            acc = acc + w[:, i]
        assert acc.tobytes() == ((f32(1) - f) + f).tobytes(), (I, O, ac)


# ---- 5. hygiene ----------------------------------------------------------------------------------------------------------------------------
def test_the_header_is_plain_code_for_host_and_device():
    with open(HEADER) as fh:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", fh.read(), flags=re.S)
    assert set(re.findall(r"#include\s*(\S+)", text)) <= {"<math.h>", "<stdint.h>"}
    assert not re.search(r"\bgetenv\b", text)


def test_the_sanitizer_sweep_builds_and_finds_nothing():
    r = subprocess.run(["make", "-s", "-C", WRAP, "sweep"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "no finding" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
