"""Keeps csrc/head_select.h honest without a GPU: the compiled header (tests/head_select_host) against the Python restatement in
tests/_headref.py on both sides of every gate -- C % 4, each pixel stride, each pointer's alignment, a NULL dx --, the argument
predicate, the header being plain host code, and the launchers of csrc/head_ops.hip noting the selector's names only."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

import _headref as R

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "head_select_host")
CSRC = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
X, DX = 0x10000, 0x20000


@pytest.fixture(scope="module")
def sel():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libhead_select.so"))
    so.hs_name.restype = C.c_char_p
    so.hs_const.restype = C.c_longlong
    so.hs_vec_ok.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int]
    so.hs_select.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_double)]
    return so


def select(so, backward, Cc, x, ldx, dx=0, lddx=0):
    o = (C.c_double * 3)()
    so.hs_select(int(backward), Cc, x, ldx, dx, lddx, o)
    return so.hs_name(int(o[0])).decode(), int(o[1]), int(o[2])


def test_constants_and_names(sel):
    assert [sel.hs_const(i) for i in range(8)] == [R.TPB, R.GROUP, 16, 0, 1, 2, 3, -1]
    n = sel.hs_count()
    assert n == len(R.NAMES) == 4 and sel.hs_name(n) is None and sel.hs_name(-1) is None
    assert tuple(sel.hs_name(k).decode() for k in range(n)) == R.NAMES and len(set(R.NAMES)) == n


def test_every_gate_alone_on_both_sides(sel):
    """From a call with every gate open (16-byte accesses), closing any ONE gate gives the scalar kernel; the forward and a backward
    without dx do not look at dx's stride."""
    for backward in (False, True):
        f = "bwd" if backward else "fwd"
        dx = DX if backward else 0
        assert select(sel, backward, 64, X, 64, dx, 64) == (f"head_{f}_kernel<4>", 4, 16)
        for Cc in (1, 2, 3, 5, 6, 7, 63, 65):                                  # C % 4
            assert select(sel, backward, Cc, X, 68, dx, 68)[:2] == (f"head_{f}_kernel<1>", 1), Cc
        for Cc in (4, 8, 20, 256):
            assert select(sel, backward, Cc, X, Cc + 4, dx, Cc + 8)[:2] == (f"head_{f}_kernel<4>", 4), Cc
        for ldx in (65, 66, 67, 69):                                           # x's pixel stride
            assert select(sel, backward, 64, X, ldx, dx, 64)[1] == 1, ldx
        for off in (4, 8, 12, 20):                                             # x's base
            assert select(sel, backward, 64, X + off, 64, dx, 64)[1] == 1, off
        for off in (16, 32, 4096):
            assert select(sel, backward, 64, X + off, 64, dx, 64)[1] == 4, off
    for lddx in (65, 66, 67):                                                  # dx's pixel stride: the backward's alone ...
        assert select(sel, True, 64, X, 64, DX, lddx) == ("head_bwd_kernel<1>", 1, 16)
        assert select(sel, True, 64, X, 64, 0, lddx) == ("head_bwd_kernel<4>", 4, 16), "a NULL dx puts no condition on its stride"
        assert select(sel, False, 64, X, 64, DX, lddx) == ("head_fwd_kernel<4>", 4, 16), "the forward has no dx"
    for off in (4, 8, 12):                                                     # ... and dx's base
        assert select(sel, True, 64, X, 64, DX + off, 64)[1] == 1
        assert select(sel, False, 64, X, 64, DX + off, 64)[1] == 4
    assert select(sel, True, 64, X, 64, DX + 16, 96)[1] == 4


def test_restatement_agrees_everywhere(sel):
    for backward, Cc, pad, xoff, dmode, dpad in itertools.product((False, True), (1, 3, 4, 5, 20, 64, 65, 256), (0, 1, 2, 4), (0, 4, 8, 16),
                                                                 (None, 0, 4, 16), (0, 2, 4)):
        dx = 0 if dmode is None else DX + dmode
        got = select(sel, backward, Cc, X + xoff, Cc + pad, dx, Cc + dpad)
        assert got == R.predict(backward, Cc, X + xoff, Cc + pad, dx, Cc + dpad), (backward, Cc, pad, xoff, dmode, dpad)
        assert bool(sel.hs_vec_ok(Cc, X + xoff, Cc + pad, dx, Cc + dpad)) == R.vec_ok(Cc, X + xoff, Cc + pad, dx, Cc + dpad)
        assert got[2] * R.GROUP >= Cc > (got[2] - 1) * R.GROUP, "the channel groups cover C exactly once"


def test_the_argument_predicate_on_both_sides(sel):
    ok = lambda N, HW, Cc, ld: bool(sel.hs_shape_ok(N, HW, Cc, ld))
    assert ok(1, 1, 1, 1) and ok(128, 64, 64, 64) and ok(3, 35, 20, 21)
    assert not ok(0, 64, 64, 64) and not ok(-1, 64, 64, 64)
    assert not ok(1, 0, 64, 64) and not ok(1, 64, 0, 64)
    assert [ok(1, 1, 64, ld) for ld in (63, 64, 65)] == [False, True, True]


def test_the_selection_header_is_plain_host_code_and_the_launchers_note_its_names():
    with open(os.path.join(CSRC, "head_select.h")) as f:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
    assert not re.search(r"\bhip\w*|\bgetenv\b", text, flags=re.I)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", "<stdint.h>", '"../../include/kdcc.h"']
    with open(os.path.join(CSRC, "head_ops.hip")) as f:
        src = re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)
    assert not re.search(r'KD_NOTE_PLUMBING\(\s*"', src) and not re.search(r"\bgetenv\b", src) and "KD_NOTE_KERNEL" not in src
    assert re.findall(r"KD_NOTE_PLUMBING\(([^;]*)\);", src) == ["head_kernel_name(sel.kernel)"] * 2
    assert src.count("head_select(") == 2 and "& 15" not in src and "aligned16" not in src, "the launchers decide nothing themselves"
    assert "atomic" not in src.lower() and "workspace" not in src.lower()
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert " head_ops.hip" in mk and "$(BUILD)/head_ops.o: head_select.h" in mk


def test_the_sweep_program_builds_and_runs_clean():
    """tests/head_select_host/sweep_main.cpp, a program of its own, without the sanitizers (`make sweep` adds them)."""
    subprocess.check_call(["make", "-s", "-C", WRAP, "_build/sweep_plain"])
    out = subprocess.run([os.path.join(WRAP, "_build", "sweep_plain")], capture_output=True, text=True)
    assert out.returncode == 0 and "no finding" in out.stdout, out.stderr[-2000:]
