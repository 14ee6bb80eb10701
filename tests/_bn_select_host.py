"""The host build of csrc/bn_select.h (tests/bn_select_host/wrap.cpp) for the tests that question it: tests/test_bn_select_host.py
and tests/test_nhwc_support_host.py.  load() builds and opens it; call() / bwd() return a selector's answer as a dict."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "bn_select_host")
FIELDS = ("kernel", "vec", "part_vec", "nrb", "part_x", "part_y", "finish", "grid")
BASE = 0x10000           # a buffer's base (the allocator's are 256-B aligned)
i32, i64, u64, out = C.c_int, C.c_longlong, C.c_ulonglong, C.POINTER(C.c_double)
OPERANDS = ("gy", "x", "y", "res", "dx")


def load():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libbn_select.so"))
    so.bl_name.restype = C.c_char_p
    so.bl_const.restype = i64
    so.bl_grid.restype, so.bl_grid.argtypes = C.c_uint, [i64]
    so.bl_view_ok.argtypes = [i32, i64, i32]
    so.bl_vec_ok.argtypes = [i32, i32, i64, i32, i64, i32]
    so.bl_workspace.restype, so.bl_workspace.argtypes = u64, [i64, i32]
    so.bl_sums_offset.restype, so.bl_sums_offset.argtypes = u64, [i64, i32]
    so.bl_fwd.argtypes = [i32] + [i64, i32] * 2 + [i64, i32, out]
    so.bl_bwd.argtypes = [i32] + [i64, i32] * 5 + [i64, i32, out]
    return so


def call(lib, fn, *args):
    o = (C.c_double * len(FIELDS))()
    getattr(lib, "bl_" + fn)(*args, o)
    sel = {k: int(v) for k, v in zip(FIELDS, o)}
    sel["name"] = lib.bl_name(sel["kernel"]).decode()
    return sel


def bwd(lib, es, M, Cc, views):
    """views: operand -> (pointer value, ld); an operand that is not named is absent."""
    args = []
    for name in OPERANDS:
        args += list(views.get(name, (0, 0)))
    return call(lib, "bwd", es, *args, M, Cc)
