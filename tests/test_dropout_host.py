"""Keeps the dropout rule (csrc/dropout_rng.h) and the kernel selection (csrc/dropout_select.h) honest without a GPU: the compiled
headers (tests/dropout_select_host) against the generator's known answers and the numpy / Python restatements in tests/_dropoutref.py
-- the keep decision at indices above 2^34, offsets above 2^32 and seeds above 2^63; both sides of every selector gate, each alone;
the grid at its cap and one item over it --, the headers being plain host code, the launcher noting the selector's names only, and
the plumbing: the declaration, the export, the ctypes signature and the argument checks of ops.dropout_nhwc."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _dropoutref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WRAP = os.path.join(HERE, "dropout_select_host")
PKG = os.path.join(ROOT, "knowledge-distillation-by-replacing-cheap-conv_amd")
CSRC = os.path.join(PKG, "csrc")
X, Y = 0x10000, 0x20000
KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
RATES = (0.2, 0.25, 0.3, 0.85)


@pytest.fixture(scope="module")
def so():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libdropout_select.so"))
    u32p = C.POINTER(C.c_uint32)
    so.dr_philox.argtypes = [u32p, u32p, u32p]
    so.dr_const.restype = so.ds_const.restype = so.ds_grid.restype = C.c_longlong
    so.dr_keep.argtypes = [C.c_uint64, C.c_uint64, C.c_int64, C.c_uint32]
    so.dr_keep_many.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p]
    so.dr_apply.argtypes, so.dr_apply.restype = [C.c_float, C.c_int, C.c_float], C.c_float
    so.ds_name.restype = C.c_char_p
    so.ds_args_ok.argtypes = [C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.c_int]
    so.ds_vec_ok.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int]
    so.ds_grid.argtypes = [C.c_longlong]
    so.ds_select.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_double)]
    return so


def philox(so, ctr, key):
    o = (C.c_uint32 * 4)()
    so.dr_philox((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), o)
    return tuple(o)


def keep_many(so, seed, offset, idx, threshold):
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    out = np.empty(idx.size, dtype=np.uint8)
    so.dr_keep_many(seed, offset, idx.ctypes.data, idx.size, threshold, out.ctypes.data)
    return out.astype(bool)


def select(so, dtype, M, Cc, x, ldx, y, ldy):
    o = (C.c_double * 4)()
    so.ds_select(dtype, M, Cc, x, ldx, y, ldy, o)
    return so.ds_name(int(o[0])).decode(), int(o[1]), int(o[2]), int(o[3])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_known_answers_through_the_compiled_header_and_the_restatement(so):
    assert [so.dr_const(i) for i in range(7)] == [0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 10, 4, -1]
    for ctr, key, want in KNOWN:
        assert philox(so, ctr, key) == want
        assert tuple(int(w) for w in R.philox4x32_10(ctr, key)) == want


def test_the_generator_agrees_with_the_restatement_on_random_counters(so):
    rng = np.random.default_rng(7)
    for _ in range(200):
        ctr, key = tuple(int(v) for v in rng.integers(0, 1 << 32, 4)), tuple(int(v) for v in rng.integers(0, 1 << 32, 2))
        assert philox(so, ctr, key) == tuple(int(w) for w in R.philox4x32_10(ctr, key))


@pytest.mark.parametrize("p", RATES)
def test_keep_decision_against_the_restatement(so, p):
    """idx below and above 2^34 (the counter's second word in use), offset below and above 2^32, seed above 2^63."""
    threshold = R.params(p)[0]
    assert threshold == int(p * 2 ** 32) and 0 < threshold < 2 ** 32
    spans = [np.arange(0, 4099), np.arange(2 ** 32 - 9, 2 ** 32 + 9), np.arange(2 ** 34 - 2050, 2 ** 34 + 2051),
             np.arange(2 ** 40 + 1, 2 ** 40 + 300), np.arange(2 ** 62 - 5, 2 ** 62 + 6)]
    idx = np.concatenate(spans).astype(np.int64)
    kept_share = []
    for seed, offset in itertools.product((0, 123, 2 ** 32 + 5, 2 ** 63 + 12345, 2 ** 64 - 1), (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 64 - 1)):
        got = keep_many(so, seed, offset, idx, threshold)
        want = R.keep(seed, offset, idx, threshold)
        assert np.array_equal(got, want), (seed, offset)
        kept_share.append(got.mean())
        assert bool(so.dr_keep(seed, offset, int(idx[5]), threshold)) == bool(want[5])
    assert abs(np.mean(kept_share) - (1 - p)) < 0.01          # (30 x 8.8k draws: sigma < 0.001)


def test_the_mask_depends_on_seed_offset_and_index_only(so):
    idx = np.arange(4096, dtype=np.int64)
    a = keep_many(so, 123, 0, idx, R.params(0.3)[0])
    assert not np.array_equal(a, keep_many(so, 123, 1, idx, R.params(0.3)[0]))
    assert not np.array_equal(a, keep_many(so, 124, 0, idx, R.params(0.3)[0]))
    assert not np.array_equal(a, keep_many(so, 123 + 2 ** 32, 0, idx, R.params(0.3)[0])), "the seed's high word is key word 1"
    assert not np.array_equal(a, keep_many(so, 123, 2 ** 32, idx, R.params(0.3)[0])), "the offset's high word is counter word 3"
    assert np.array_equal(a, R.mask(123, 0, 256, 16, 0.3).reshape(-1)) and np.array_equal(a, R.mask(123, 0, 4096, 1, 0.3).reshape(-1))
    assert keep_many(so, 123, 0, idx, 0).all(), "p = 0 keeps every element"


def test_the_value_rule(so):
    s = float(R.params(0.3)[1])
    for x in (1.5, -2.25, 0.0, 1.0e38, 1e-40):
        assert np.float32(so.dr_apply(x, 1, s)) == np.float32(x) * np.float32(s)
        assert so.dr_apply(x, 0, s) == 0.0 and not np.signbit(np.float32(so.dr_apply(-abs(x), 0, s)))
    x = np.array([1.0, -3.0, 0.5, 7.0], dtype=np.float32)
    assert np.array_equal(R.apply_f32(x, np.array([True, False, True, False]), 0.3), np.array([x[0] * np.float32(s), 0, x[2] * np.float32(s), 0], np.float32))
    # bf16: the float32 product rounded to nearest-even once -- torch's own cast is the witness
    t = torch.randn(4096, generator=torch.Generator().manual_seed(3)).bfloat16()
    bits = t.view(torch.int16).numpy().view(np.uint16)
    want = (t.float() * torch.tensor(R.params(0.3)[1])).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.apply_bf16(bits, np.ones(4096, bool), 0.3), want)


# ---- the selection ----------------------------------------------------------------------------------------------------------------
def test_constants_and_names(so):
    assert [so.ds_const(i) for i in range(9)] == [R.TPB, R.CAP, R.VEC_BYTES, R.BLOCK, 0, 1, 2, 3, -1]
    n = so.ds_count()
    assert n == len(R.NAMES) == 4 and so.ds_name(n) is None and so.ds_name(-1) is None
    assert tuple(so.ds_name(k).decode() for k in range(n)) == R.NAMES and len(set(R.NAMES)) == n


def test_every_gate_alone_on_both_sides(so):
    """From a call with every gate open (16-byte accesses), closing any ONE gate gives the scalar kernel."""
    for dtype, v, vname, sname in ((R.F32, 4, R.NAMES[1], R.NAMES[0]), (R.BF16, 8, R.NAMES[3], R.NAMES[2])):
        es = 16 // v
        assert select(so, dtype, 128, 64, X, 64, Y, 64) == (vname, v, 128 * 64 // v, 128 * 64 // v // R.TPB)
        assert select(so, dtype, 128, 64, X, 64, X, 64)[:2] == (vname, v), "in place"
        for Cc in (1, 2, 3, 5, 6, 7, 10, 63, 65, 4 if v == 8 else 7, 12 if v == 8 else 9):       # C % vector width
            assert select(so, dtype, 128, Cc, X, 64 + 8, Y, 64 + 8)[:2] == (sname, 1), Cc
        for Cc in (8, 16, 64, 160, 256):
            assert select(so, dtype, 128, Cc, X, Cc + 8, Y, Cc + 16)[:2] == (vname, v), Cc
        for ld in (65, 66, 67, 69, 64 + v // 2, 64 + v - 1):                                          # each pixel stride
            assert select(so, dtype, 128, 64, X, ld, Y, 64)[:2] == (sname, 1), ld
            assert select(so, dtype, 128, 64, X, 64, Y, ld)[:2] == (sname, 1), ld
        for ld in (64 + v, 96, 192):
            assert select(so, dtype, 128, 64, X, ld, Y, 64)[1] == v and select(so, dtype, 128, 64, X, 64, Y, ld)[1] == v
        for off in (es, 2 * es, 8, 12, 16 - es):                                                      # each base
            assert select(so, dtype, 128, 64, X + off, 64, Y, 64)[:2] == (sname, 1), off
            assert select(so, dtype, 128, 64, X, 64, Y + off, 64)[:2] == (sname, 1), off
        for off in (16, 32, 4096):
            assert select(so, dtype, 128, 64, X + off, 64, Y, 64)[1] == v and select(so, dtype, 128, 64, X, 64, Y + off, 64)[1] == v
    assert select(so, R.F32, 128, 4, X, 4, Y, 4)[0] == R.NAMES[1] and select(so, R.BF16, 128, 4, X, 8, Y, 8)[0] == R.NAMES[2], \
        "4 channels are a whole access in fp32 only"


def test_the_grid_at_its_cap_and_one_item_over(so):
    full = R.CAP * R.TPB
    assert [so.ds_grid(i) for i in (0, 1, R.TPB, R.TPB + 1, full - R.TPB, full - R.TPB + 1, full, full + 1, 1 << 40)] == \
        [1, 1, 1, 2, R.CAP - 1, R.CAP, R.CAP, R.CAP, R.CAP]
    # through the selector: vector items are pixel-channel groups, scalar items Philox blocks (the last may be partial)
    assert select(so, R.F32, full, 4, X, 4, Y, 4)[2:] == (full, R.CAP)
    assert select(so, R.F32, full + 1, 4, X, 4, Y, 4)[2:] == (full + 1, R.CAP), "one item over: the grid stays, the kernel strides"
    assert select(so, R.F32, full - R.TPB, 4, X, 4, Y, 4)[2:] == (full - R.TPB, R.CAP - 1)
    assert select(so, R.F32, 105, 10, X, 10, Y, 10)[2:] == (263, 2), "1050 elements: 262 blocks and a half"
    assert select(so, R.BF16, 128, 160, X, 192, Y, 192)[2:] == (128 * 20, 10)
    assert select(so, R.F32, 1 << 33, 5, X, 5, Y, 5)[2:] == (5 * (1 << 33) // 4, R.CAP), "items past 2^32"


def test_restatement_agrees_everywhere(so):
    for dtype, Cc, padx, pady, xoff, yoff, M in itertools.product((R.F32, R.BF16), (1, 3, 4, 8, 10, 16, 20, 160, 161), (0, 1, 2, 4, 8, 32), (0, 4, 8),
                                                                  (0, 4, 8, 16), (0, 2, 16), (1, 105, 128, 600000)):
        args = (dtype, M, Cc, X + xoff, Cc + padx, Y + yoff, Cc + pady)
        if not so.ds_args_ok(X + xoff, Cc + padx, Y + yoff, Cc + pady, dtype, M, Cc):
            assert dtype == R.F32 and yoff == 2, "only a base off its element is refused here"
            continue
        got = select(so, *args)
        assert got == R.predict(*args), args
        assert bool(so.ds_vec_ok(dtype, Cc, X + xoff, Cc + padx, Y + yoff, Cc + pady)) == R.vec_ok(dtype, Cc, X + xoff, Cc + padx, Y + yoff, Cc + pady)
        per = got[1] if got[1] > 1 else R.BLOCK
        assert got[2] * per >= M * Cc > (got[2] - 1) * per, "the items cover M * C exactly once"


def test_the_argument_predicate_on_both_sides(so):
    ok = lambda x=X, ldx=64, y=Y, ldy=64, dtype=R.F32, M=128, Cc=64: bool(so.ds_args_ok(x, ldx, y, ldy, dtype, M, Cc))
    assert ok() and ok(dtype=R.BF16) and ok(y=X) and ok(M=1, Cc=1, ldx=1, ldy=1)
    assert not ok(dtype=2) and not ok(dtype=-1)
    assert not ok(x=0) and not ok(y=0)
    assert not ok(x=X + 2) and ok(x=X + 2, dtype=R.BF16) and not ok(y=Y + 1, dtype=R.BF16) and ok(x=X + 4)
    assert not ok(M=0) and not ok(M=-1) and not ok(Cc=0)
    assert [ok(ldx=ld) for ld in (63, 64, 65)] == [False, True, True] and [ok(ldy=ld) for ld in (63, 64, 65)] == [False, True, True]
    assert ok(M=(2 ** 61 - 1) // 64) and not ok(M=(2 ** 61 - 1) // 64 + 1), "offsets and indices an int64 holds, with room to stride"


def _code(path):
    with open(path) as f:
        return re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_headers_are_plain_host_code_and_the_launcher_notes_the_selectors_names():
    sel, rng = _code(os.path.join(CSRC, "dropout_select.h")), _code(os.path.join(CSRC, "dropout_rng.h"))
    assert not re.search(r"\bhip\w*|\bgetenv\b|__global__", sel, flags=re.I)
    assert re.findall(r"#include\s*(\S+)", sel) == ["<stddef.h>", "<stdint.h>", '"../../include/kdcc.h"']
    # the rule: no HIP calls (the one mention of the compiler is the macro that marks its functions for both sides), no state
    assert re.findall(r"#include\s*(\S+)", rng) == ["<stdint.h>"]
    body = re.sub(r"#if defined\(__HIPCC__\).*?#endif", "", rng, flags=re.S)
    assert not re.search(r"\bhip\w*|\bgetenv\b|__global__|__device__|__shared__|\bstatic\b(?! inline)", body, flags=re.I)
    for text in (sel, rng):
        statics = re.findall(r"^\s*static\s+(?!inline\b|const char \*const names\[\]|_?assert)[^\n]*", re.sub(r"static_assert", "_assert", text), flags=re.M)
        assert not statics, statics
        assert not re.findall(r"^(?!\s*(?:constexpr|static|struct|enum|typedef|#|DROPOUT_FN|\}|\{|$))\S[^\n(]*;\s*$", text, flags=re.M), "a global"
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):
        assert word.lower() in rng.lower()
    src = _code(os.path.join(CSRC, "dropout.hip"))
    assert not re.search(r'KD_NOTE_PLUMBING\(\s*"', src) and not re.search(r"\bgetenv\b", src) and "KD_NOTE_KERNEL" not in src
    assert re.findall(r"KD_NOTE_PLUMBING\(([^;]*)\);", src) == ["dropout_kernel_name(sel.kernel)"]
    assert src.count("dropout_select(") == 1 and src.count("dropout_args_ok(") == 1
    assert "& 15" not in src and "aligned(" not in src and "aligned16" not in src and "% 4" not in src and "% 8" not in src, "the launcher decides nothing itself"
    assert "atomic" not in src.lower() and "workspace" not in src.lower() and "__shared__" not in src
    assert '#include "dropout_rng.h"' in src and "philox4x32_10(" not in src.replace("dropout_rng.h", ""), "one rule: the header's"
    for name in R.NAMES:          # every name of the table is an instantiation the launcher launches
        assert f"({name})" in src, name
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert " dropout.hip" in mk and "$(BUILD)/dropout.o: dropout_rng.h dropout_select.h" in mk
    assert not [f for f in os.listdir(CSRC) if f.startswith("bn_") and "dropout" in f]


def test_the_sweep_program_builds_and_runs_clean():
    """tests/dropout_select_host/sweep_main.cpp, a program of its own, without the sanitizers (`make sweep` adds them)."""
    subprocess.check_call(["make", "-s", "-C", WRAP, "_build/sweep_plain"])
    out = subprocess.run([os.path.join(WRAP, "_build", "sweep_plain")], capture_output=True, text=True)
    assert out.returncode == 0 and "no finding" in out.stdout, out.stderr[-2000:]


# ---- the plumbing -----------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_listed():
    from kdcc_amd import _lib
    with open(os.path.join(ROOT, "include", "kdcc.h")) as f:
        hdr = f.read()
    m = re.search(r"int kd_dropout_nhwc\(([^;]*)\);", hdr)
    assert m, "kd_dropout_nhwc is not declared in include/kdcc.h"
    types = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]
    assert types == ["const void *", "int32_t", "void *", "int32_t", "int32_t", "int64_t", "int32_t", "uint32_t", "float", "uint64_t", "uint64_t",
                     "kd_stream_t"]
    assert "Philox4x32-10" in hdr and "idx >> 2" in hdr and "word >= threshold" in hdr, "the rule belongs in the declaration's comment"
    res, args = _lib._SIGS["kd_dropout_nhwc"]
    assert res is C.c_int32 and args == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_uint32, C.c_float,
                                         C.c_uint64, C.c_uint64, C.c_void_p]
    assert "kd_dropout_nhwc" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "kd_dropout_nhwc"), "the library does not export kd_dropout_nhwc"
    assert not [s for s in _lib.exported_symbols() if "dropout" in s and "workspace" in s]


def test_ops_refuses_host_tensors_and_rates_outside_the_half_open_interval():
    from kdcc_amd import ops
    from kdcc_amd._lib import KdccError
    x = torch.zeros(1, 2, 2, 4)
    with pytest.raises(KdccError):
        ops.dropout_nhwc(x, 0.3, 0, 0)
    for p in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.dropout_nhwc(x, p, 0, 0)
    assert ops.dropout_params(0.0) == (0, 1.0)
    for p in RATES:
        thr, scale = ops.dropout_params(p)
        assert (thr, np.float32(scale)) == R.params(p)


def test_the_stream_follows_torchs_seed_and_the_identity_cases_draw_nothing():
    from kdcc_amd import nn_hip
    keep = torch.initial_seed()
    try:
        torch.manual_seed(1234)
        assert nn_hip.dropout_state() == (1234, 0)
        x = torch.zeros(1, 4, 2, 2)
        assert nn_hip.dropout(x, 0.3, False) is x and nn_hip.dropout(x, 0.0, True) is x
        assert nn_hip.dropout_state() == (1234, 0), "the identity draws nothing"
        assert nn_hip._dropout_draw() == (1234, 0) and nn_hip._dropout_draw() == (1234, 1) and nn_hip.dropout_state() == (1234, 2)
        nn_hip.seed_dropout(2 ** 63 + 5, 2 ** 32)
        assert nn_hip.dropout_state() == (2 ** 63 + 5, 2 ** 32) and nn_hip._dropout_draw() == (2 ** 63 + 5, 2 ** 32)
        assert nn_hip.dropout_state() == (2 ** 63 + 5, 2 ** 32 + 1)
        torch.manual_seed(1234)          # (the same seed again: torch's seed has not changed, the stream goes on)
        assert nn_hip.dropout_state() == (2 ** 63 + 5, 2 ** 32 + 1)
        torch.manual_seed(99)
        assert nn_hip.dropout_state() == (99, 0), "a new torch seed restarts the stream"
        with pytest.raises(ValueError):
            nn_hip.seed_dropout(-1)
        with pytest.raises(ValueError):
            nn_hip.dropout(x, 1.0, True)
        nn_hip.allow_host_tensors(True)
        try:
            with pytest.raises(NotImplementedError, match="dropout"):
                nn_hip.dropout(x, 0.3, True)
        finally:
            nn_hip.allow_host_tensors(False)
        assert nn_hip.dropout_state() == (99, 0)
    finally:
        torch.manual_seed(keep)
