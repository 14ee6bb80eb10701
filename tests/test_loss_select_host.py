"""The criterion selection the library really runs (csrc/loss_select.h: one selector per family, the grids, the LDS budgets, the
workspace), compiled for the host and held against the restatement of tests/_loss_dispatch_cases.py -- without a GPU.
Four things: the kernel and the grid of every row of the GPU test's case table; selector against rule on synthesised calls over
every layout, dtype triple and class count on both sides of every numeric gate (computed from the header's constants); the name
table and the header's hygiene; the workspace against the parent's formula."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import _loss_dispatch_cases as L

HERE = os.path.dirname(os.path.abspath(__file__))
WRAP = os.path.join(HERE, "loss_select_host")
CSRC = os.path.join(os.path.dirname(HERE), "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
FIELDS = ("kernel", "why", "blocks", "lds", "cpr", "nchunks", "chunks", "per_chunk", "aux_off", "sh", "sw", "oh", "ow")
WHY_NONE, WHY_CLASSES, WHY_SPAN, WHY_TOPK_MAX_C = range(4)
KINDS = ("kld", "jsd", "ekl")
UP_OPS = ("ce2d_up", "kldiv_up", "jsdiv_up", "focal_up", "metrics_up")
DTS = ("f32", "bf16")
BASE = 0x10000           # a buffer's base (the allocator's are 256-B aligned); a slice starts 8 elements in, "off1" one element
REFUSED = "(refused)"
View = C.c_longlong * 5


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", WRAP])
    so = C.CDLL(os.path.join(WRAP, "_build", "libloss_select.so"))
    so.ls_name.restype = C.c_char_p
    so.ls_const.restype = C.c_longlong
    so.ls_blocks_for.argtypes = [C.c_longlong]
    so.ls_workspace.restype = so.ls_topk_workspace.restype = C.c_ulonglong
    so.ls_workspace.argtypes = so.ls_topk_workspace.argtypes = [C.c_int, C.c_int, C.c_longlong]
    out, v, ncp = C.POINTER(C.c_double), C.POINTER(C.c_longlong), [C.c_int, C.c_int, C.c_longlong]
    so.ls_pair.argtypes = [C.c_int, v, v, v] + ncp + [out]
    so.ls_mse.argtypes = [v, v, v] + ncp + [out]
    so.ls_whmse.argtypes = ncp + [out]
    so.ls_ce2d.argtypes = so.ls_confusion.argtypes = [v] + ncp + [out]
    so.ls_up.argtypes = [C.c_int] * 8 + [out]
    so.ls_topk.argtypes = [v, v, v, C.c_longlong, C.c_longlong] + ncp + [out]
    so.ls_multi.argtypes = [v, v, C.c_int, v, C.c_int] + ncp + [out]
    so.ls_scale.argtypes = [C.c_int, C.c_longlong, out]
    return so


def consts(lib):
    names = ("MAX_BLOCKS", "FOCAL_MAX_BLOCKS", "MT_MAX_BLOCKS", "MET_MAX_BLOCKS", "UP_NW", "TOPK_MAX_C", "LDS")
    return {n: lib.ls_const(i) for i, n in enumerate(names)}


def view(lay, dt, shape):
    """The five integers of a view: a pointer value with the alignment the layout's base has, the dtype, L.strides."""
    esz = 2 if dt == "bf16" else 4
    ptr = BASE + {"off1": esz, "cs": 8 * esz, "2ds": 8 * esz}.get(lay, 0)
    assert (ptr % 16 == 0) == L.aligned16(lay, dt)
    return View(ptr, DTS.index(dt), *L.strides(lay, shape))


def call(lib, fn, *args):
    out = (C.c_double * len(FIELDS))()
    getattr(lib, fn)(*args, out)
    sel = dict(zip(FIELDS, out))
    for k in FIELDS[:9]:
        sel[k] = int(sel[k])
    sel["name"] = REFUSED if sel["kernel"] == lib.ls_refused() else lib.ls_name(sel["kernel"]).decode()
    return sel


def three(c):
    """(s, t, grad or None) views of a two-operand row."""
    ls, lt, lg = L.lays(c)
    gdt = c.get("gdt", c["sdt"])
    return view(ls, c["sdt"], c["shape"]), view(lt, c["tdt"], c["shape"]), (view(lg, gdt, c["shape"]) if gdt else None)


def select(lib, c):
    """The selector of the row's family on the row's views and dims."""
    op = c["op"]
    if op in UP_OPS:
        return call(lib, "ls_up", UP_OPS.index(op), *c["geom"], int(c["ac"]))
    N, Cc, P = L.dims(c)
    if op == "pair":
        return call(lib, "ls_pair", KINDS.index(c["kind"]), *three(c), N, Cc, P)
    if op == "hint_mse":
        return call(lib, "ls_mse", *three(c), N, Cc, P)
    if op == "topk":       # no mask of the caller's: the kernel's own, in a 256-B aligned workspace
        return call(lib, "ls_topk", *three(c), 0, 2 * BASE, N, Cc, P)
    if op in ("ce2d", "confusion"):
        return call(lib, "ls_" + op, view(c["lay"], c["dt"], c["shape"]), N, Cc, P)
    assert op in ("kldiv_multi", "softmax_mean")
    # every operand in the row's layout (L.multi_rule: the gradient / the fp32 output answer the three questions like the first operand)
    smean = op == "softmax_mean"
    ts = (C.c_longlong * (5 * c["nt"]))(*(list(view(c["lay"], c["dt"], c["shape"])) * c["nt"]))
    g = view(c["lay"], "f32" if smean else c["dt"], c["shape"]) if smean or c.get("grad", True) else None
    return call(lib, "ls_multi", None if smean else view(c["lay"], c["dt"], c["shape"]), ts, c["nt"], g, int(smean), N, Cc, P)


def refused_before_selection(c):
    """Rows an argument check of the entry point refuses before it selects (the selector never sees K or a bad operand count)."""
    return (c["op"] == "topk" and not 1 <= c["k"] <= c["shape"][1]) or (c["op"] in ("kldiv_multi", "softmax_mean") and not 1 <= c["nt"] <= L.KD_MULTI_MAX)


def restated_blocks(c, name):
    """The grid of the launch the row names, from the restatements of the case table."""
    if c["op"] in UP_OPS:
        return min(L.up_chunks(c), L.UP_CAP[c["op"]])
    N, Cc, P = L.dims(c)
    if c["op"] in ("kldiv_multi", "softmax_mean"):
        return min((N * P + 3) // 4 if name.startswith("mt_wave") else (N * P + 255) // 256, L.MT_MAX_BLOCKS)
    if c["op"] in ("hint_mse", "topk"):
        return 0 if name == "topk_nograd" else L.blocks_for(N * Cc * P // 8 if "_vec_" in name else N * Cc * P)
    return L.blocks_for(N * P)


def restated_lds(c, name):
    """The dynamic LDS of the launch the row names, from the budgets the case table's rules compare with the limit."""
    if c["op"] in UP_OPS:
        Cc = c["geom"][3]
        return (2 if c["op"] in ("ce2d_up", "focal_up") else 4) * L.UP_NW * Cc * 4 + (2 * Cc * Cc * 4 if c["op"] == "metrics_up" else 0)
    Cc = L.dims(c)[1]
    per_thread = {"pair_nhwc_kernel": 2, "ce2d_nhwc_kernel": 1, "confusion_nhwc_kernel": 1, "kldm_nhwc_kernel": 3}.get(name.split("<")[0], 0)
    return per_thread * 256 * Cc * 4 + (Cc * Cc * 4 if c["op"] == "confusion" else 0)


RULED = [c for c in L.CASES if c["op"] in L.RULES]


def test_the_header_and_the_case_table_agree_on_the_constants(lib):
    K = consts(lib)
    assert K == {"MAX_BLOCKS": L.MAX_BLOCKS, "FOCAL_MAX_BLOCKS": L.FOCAL_MAX_BLOCKS, "MT_MAX_BLOCKS": L.MT_MAX_BLOCKS, "MET_MAX_BLOCKS": L.MET_MAX_BLOCKS,
                 "UP_NW": L.UP_NW, "TOPK_MAX_C": 4096, "LDS": L.LDS}
    for i, op in enumerate(UP_OPS):
        assert (lib.ls_up_max_classes(i), lib.ls_up_max_blocks(i)) == (L.UP_LIMIT[op], L.UP_CAP[op])
    for total in (-5, 0, 1, 256, 257, 2048 * 256, 2048 * 256 + 1, 1 << 40):
        assert lib.ls_blocks_for(total) == L.blocks_for(total)


@pytest.mark.parametrize("c", RULED, ids=L.ids(RULED))
def test_every_ruled_row_selects_its_kernel_on_its_grid(lib, c):
    if refused_before_selection(c):
        assert c["kernel"] == REFUSED == L.rule(c)
        return
    sel = select(lib, c)
    assert sel["name"] == c["kernel"], f"{c['id']}: loss_select.h picks {sel['name']}, the row says {c['kernel']}"
    if c["kernel"] == REFUSED:
        assert sel["why"] in (WHY_CLASSES, WHY_SPAN)
        return
    assert sel["why"] == WHY_NONE and sel["blocks"] == restated_blocks(c, sel["name"]), c["id"]
    assert sel["lds"] == restated_lds(c, sel["name"]) <= (160 * 1024 if c["op"] == "metrics_up" else L.LDS), c["id"]
    if "second_trip" in c:       # the grid the launch really gets is the cap the row claims, and the row's work exceeds it
        work, cap = c["second_trip"]
        assert sel["blocks"] == cap and work > cap * 256


def test_every_row_refused_for_its_classes_or_its_span_says_so(lib):
    for c in RULED:
        if c["op"] in UP_OPS and c["kernel"] == REFUSED:
            assert select(lib, c)["why"] == (WHY_CLASSES if c["geom"][3] > L.UP_LIMIT[c["op"]] else WHY_SPAN), c["id"]


# ---- selector against rule on synthesised calls ----------------------------------------------------------------------------------------
LAYS4, LAYS2 = ("nchw", "cl", "off1", "cs", "bs"), ("2d", "2ds")
TRIPLES = [(s, t, g) for s in DTS for t in DTS for g in DTS + (None,)]


def agree(lib, c):
    c.setdefault("id", "synthetic")
    sel, want = select(lib, c), L.rule(c)
    got = sel["name"]
    assert got == want, f"loss_select.h picks {got}, the restated gate {want}: {c}"
    assert got == REFUSED or sel["lds"] == restated_lds(c, got) <= (160 * 1024 if c["op"] == "metrics_up" else L.LDS), c
    return got


def test_pair_sweep(lib):
    K = consts(lib)
    fits = K["LDS"] // (2 * 256 * 4)                      # classes whose two staged vectors per thread fit the default LDS
    assert 2 * 256 * 4 * fits <= K["LDS"] < 2 * 256 * 4 * (fits + 1)
    seen = set()
    for kind, (sdt, tdt, gdt), Cc, N in itertools.product(KINDS, TRIPLES, (19, fits, fits + 1), (1, 2)):
        lays = [(l, l, l) for l in LAYS4] + [tuple("cs" if i == j else "cl" for i in range(3)) for j in range(3)] + [("cl", "cl", "bs")]
        for lay in lays:
            seen.add(agree(lib, dict(op="pair", kind=kind, shape=(N, Cc, 3, 5), lay=lay if gdt else lay[:2] + (None,), sdt=sdt, tdt=tdt, gdt=gdt)))
        for lay in LAYS2:
            seen.add(agree(lib, dict(op="pair", kind=kind, shape=(N + 5, Cc), lay=lay, sdt=sdt, tdt=tdt, gdt=gdt)))
    assert len(seen) == 27
    for kind in KINDS:         # the gate itself: the last class count that fits, the first that does not
        names = [agree(lib, dict(op="pair", kind=kind, shape=(2, Cc, 3, 5), lay="cl", sdt="f32", tdt="f32", gdt="f32")) for Cc in (fits, fits + 1)]
        assert names == [f"pair_nhwc_kernel<{kind},f32,f32,f32>", f"pair_kernel<{kind}>"]


def test_ce2d_and_confusion_sweep(lib):
    K = consts(lib)
    ce_fits = K["LDS"] // (256 * 4)
    cf_fits = max(Cc for Cc in range(1, 65) if 256 * Cc * 4 + Cc * Cc * 4 <= K["LDS"])
    assert (ce_fits, cf_fits) == (64, 53)
    for op, fits in (("ce2d", ce_fits), ("confusion", cf_fits)):
        for dt, Cc, N in itertools.product(DTS, (19, fits, fits + 1), (1, 2)):
            for lay in LAYS4:
                agree(lib, dict(op=op, shape=(N, Cc, 3, 5), lay=lay, dt=dt))
            for lay in LAYS2:
                agree(lib, dict(op=op, shape=(N + 5, Cc), lay=lay, dt=dt))
        names = [agree(lib, dict(op=op, shape=(2, Cc, 3, 5), lay="cl", dt="f32")) for Cc in (fits, fits + 1)]
        assert names == [f"{op}_nhwc_kernel<f32>", f"{op}_kernel"]


def test_mse_and_topk_sweep(lib):
    """numel % 8, C % 8 and P % 8 in {0, 1}, aligned and off-by-one-element bases, every layout and dtype triple, with and
    without a gradient."""
    seen = set()
    shapes = [(N, Cc, H, W) for N in (1, 2, 8) for Cc in (8, 9) for H, W in ((2, 4), (3, 3))]
    assert {(s[1] % 8, s[2] * s[3] % 8) for s in shapes} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {int(np.prod(s)) % 8 == 0 for s in shapes} == {True, False}
    for op, (sdt, tdt, gdt), shape in itertools.product(("hint_mse", "topk"), TRIPLES, shapes):
        lays = [(l, l, l) for l in LAYS4] + [("cl", "cl", "cs"), ("cl", "off1", "cl"), ("nchw", "nchw", "cl")]
        for lay in lays:
            seen.add(agree(lib, dict(op=op, shape=shape, lay=lay if gdt else lay[:2] + (None,), sdt=sdt, tdt=tdt, gdt=gdt, k=1)))
    for op in ("hint_mse", "topk"):
        for lay in LAYS2:
            seen.add(agree(lib, dict(op=op, shape=(8, 8), lay=lay, sdt="f32", tdt="f32", gdt="f32", k=1)))
    assert seen == {"mse_vec_kernel<f32>", "mse_vec_kernel<bf16>", "mse_strided_kernel", "topk_nograd", "topk_grad_kernel"} | {
        f"topk_grad_vec_kernel<{d},{f}>" for d in DTS for f in ("cfast", "pfast")}
    # a caller's mask that is not 16-B aligned keeps the dense gradient off the vector kernel; above TOPK_MAX_C nothing is selected
    c = dict(op="topk", shape=(2, 8, 2, 4), lay="cl", sdt="f32", tdt="f32", gdt="f32")
    for mask, want in ((0, "topk_grad_vec_kernel<f32,cfast>"), (3 * BASE, "topk_grad_vec_kernel<f32,cfast>"), (3 * BASE + 4, "topk_grad_kernel")):
        assert call(lib, "ls_topk", *three(c), mask, 2 * BASE, 2, 8, 8)["name"] == want
    assert call(lib, "ls_topk", *three(c), 0, 2 * BASE + 8, 2, 8, 8)["name"] == "topk_grad_kernel"
    top = consts(lib)["TOPK_MAX_C"]
    for Cc, why in ((top, WHY_NONE), (top + 1, WHY_TOPK_MAX_C)):
        big = dict(c, shape=(1, Cc, 1, 8))
        sel = call(lib, "ls_topk", *three(big), 0, 2 * BASE, 1, Cc, 8)
        assert (sel["name"] == REFUSED, sel["why"]) == (why != WHY_NONE, why)


def test_multi_sweep(lib):
    """C = 21 / 22 with 16383 / 16384 rows, then 256 / 257 and 1024 / 1025 (C % 4 = 0 / 1), every layout, both dtypes, 1 and 3
    operands, with and without a gradient, both entry points."""
    seen = set()
    for op, dt, nt, grad in itertools.product(("kldiv_multi", "softmax_mean"), DTS, (1, 3), (True, False)):
        for Cc, (N, H, W) in itertools.product((21, 22), ((1, 127, 129), (1, 128, 128), (2, 64, 128))):
            assert N * H * W in (16383, 16384)
            for lay in LAYS4:
                seen.add(agree(lib, dict(op=op, shape=(N, Cc, H, W), lay=lay, dt=dt, nt=nt, grad=grad)))
        for Cc in (256, 257, 1024, 1025, 1028):
            for lay in LAYS2:
                seen.add(agree(lib, dict(op=op, shape=(5, Cc), lay=lay, dt=dt, nt=nt, grad=grad)))
            for lay in LAYS4:
                seen.add(agree(lib, dict(op=op, shape=(2, Cc, 2, 3), lay=lay, dt=dt, nt=nt, grad=grad)))
    tails = ("", ",smean")
    assert seen == {"kldm_nhwc_kernel", "kldm_kernel", "kldm_kernel<smean>"} | {f"mt_wave_kernel<{n},{v}{t}>" for n in (1, 4) for v in ("vec", "novec") for t in tails}
    # one operand of another layout than the rest decides: a class stride anywhere ends the wave kernels, a batch slice the NHWC one
    def mixed(lays, shape, smean=False):
        N, Cc, P = shape[0], shape[1], shape[2] * shape[3]
        ts = (C.c_longlong * (5 * (len(lays) - 1)))(*[x for l in lays[1:] for x in view(l, "f32", shape)])
        return call(lib, "ls_multi", None if smean else view(lays[0], "f32", shape), ts, len(lays) - 1, view(lays[0], "f32", shape), int(smean), N, Cc, P)["name"]
    assert mixed(("cl", "cl", "cl"), (2, 24, 2, 3)) == "mt_wave_kernel<1,vec>"
    assert mixed(("cl", "cl", "nchw"), (2, 24, 2, 3)) == "kldm_kernel"
    assert mixed(("cl", "cl", "off1"), (2, 24, 2, 3)) == "mt_wave_kernel<1,novec>"
    assert mixed(("cl", "cl", "cl"), (2, 19, 64, 128)) == "kldm_nhwc_kernel"
    assert mixed(("cl", "bs", "cl"), (2, 19, 64, 128)) == "kldm_kernel"
    assert mixed(("cl", "cl", "cl"), (2, 19, 64, 128), smean=True) == "kldm_kernel<smean>"


def test_up_sweep(lib):
    """Class counts on both sides of each entry point's bound and of the 19-class specialisation, one resampling ratio on each
    side of the span gate under either alignment rule, the class count from which the metrics kernel reserves its LDS."""
    K = consts(lib)
    for op, ac in itertools.product(UP_OPS, (True, False)):
        lim = L.UP_LIMIT[op]
        for Cc in (18, 19, 20, lim, lim + 1):
            name = agree(lib, dict(op=op, geom=(2, 5, 7, Cc, 9, 14), ac=ac))
            assert name == (REFUSED if Cc > lim else L.UP_NAME[op].format(19 if Cc == 19 else 0))
        # W = 300 output columns: the widest source that still fits UP_NW staged columns, and the next
        W = 300
        spans = {w: int(np.float32(255.0) * (np.float32(w - 1) / np.float32(W - 1) if ac else np.float32(w) / np.float32(W))) + 3 for w in range(2, 2 * W)}
        w_ok = max(w for w, s in spans.items() if s <= K["UP_NW"])
        assert spans[w_ok + 1] > K["UP_NW"]
        for w, refused in ((w_ok, False), (w_ok + 1, True)):
            c = dict(op=op, geom=(1, 5, w, 3, 5, W), ac=ac)
            assert (agree(lib, c) == REFUSED) == refused
            assert select(lib, c)["why"] == (WHY_SPAN if refused else WHY_NONE)
    lds = lambda Cc: 4 * K["UP_NW"] * Cc * 4 + 2 * Cc * Cc * 4
    first = min(Cc for Cc in range(1, 49) if lds(Cc) > K["LDS"])
    assert first == 24
    for Cc in (first - 1, first, 48):
        sel = select(lib, dict(op="metrics_up", geom=(1, 5, 7, Cc, 9, 14), ac=True))
        assert sel["lds"] == lds(Cc) and (sel["lds"] > K["LDS"]) == (Cc >= first) and sel["lds"] <= 160 * 1024
    for op in UP_OPS[:4]:      # the others never ask for more than the default limit
        Cc = L.UP_LIMIT[op]
        sel = select(lib, dict(op=op, geom=(1, 5, 7, Cc, 9, 14), ac=True))
        assert sel["lds"] == (2 if op in ("ce2d_up", "focal_up") else 4) * K["UP_NW"] * Cc * 4 <= K["LDS"]
    # the geometry the kernels take: F.interpolate's source coordinate = output coordinate * s + o
    sel = select(lib, dict(op="ce2d_up", geom=(2, 5, 7, 19, 9, 14), ac=True))
    assert (sel["sh"], sel["sw"], sel["oh"], sel["ow"]) == (np.float32(4) / np.float32(8), np.float32(6) / np.float32(13), 0.0, 0.0)
    sel = select(lib, dict(op="ce2d_up", geom=(2, 5, 7, 19, 9, 14), ac=False))
    sh, sw = np.float32(5) / np.float32(9), np.float32(7) / np.float32(14)
    assert (sel["sh"], sel["sw"], sel["oh"], sel["ow"]) == (sh, sw, np.float32(0.5) * sh - np.float32(0.5), np.float32(0.5) * sw - np.float32(0.5))
    assert (sel["cpr"], sel["nchunks"]) == (1, 18)


def test_scale_and_the_weighted_hint_plan(lib):
    for dt, n in itertools.product(DTS, (1, 7, 8, 9, 2048 * 256 * 8, 2048 * 256 * 8 + 9)):
        sel = call(lib, "ls_scale", DTS.index(dt), n)
        assert (sel["name"], sel["blocks"]) == (f"scale_by_device_scalar_kernel<{dt}>", L.blocks_for(max(n // 8, 1)))
    for c in L.cases_of("whmse"):
        N, Cc, P = L.dims(c)
        sel = call(lib, "ls_whmse", N, Cc, P)
        chunks, per, empty, last = L.whmse_plan(P)
        assert (sel["name"], sel["chunks"], sel["per_chunk"], sel["blocks"]) == ("whmse_kernel", chunks, per, chunks * -(-Cc // 256) * N) and c["plan"][:2] == (chunks, per)


# ---- names and hygiene -----------------------------------------------------------------------------------------------------------------------
def header_text():
    with open(os.path.join(CSRC, "loss_select.h")) as f:
        return re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_names_are_distinct_and_every_one_has_a_row(lib):
    n = lib.ls_refused()
    names = [lib.ls_name(k).decode() for k in range(n)]
    assert lib.ls_name(n) is None and lib.ls_name(-1) is None
    assert len(set(names)) == n >= 71
    assert set(names) == {c["kernel"] for c in L.CASES} - {REFUSED}


def test_the_selection_header_is_plain_host_code():
    text = header_text()
    assert not re.search(r"\bhip\w*|\bgetenv\b", text, flags=re.I)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", "<stdint.h>", '"../../include/kdcc.h"', '"resample.h"']


# ---- the workspace: the parent's formula (kd_loss_workspace is public ABI) -------------------------------------------------------------------
def parent_workspace(N, Cc, P):
    wh_blocks = 64 * ((Cc + 255) // 256) * N
    return 2 * max(wh_blocks, 2048) * 8 + N * 4 + 64


def parent_topk_workspace(N, Cc, P):
    if N <= 0 or Cc <= 0 or P <= 0:
        return 64
    ch = min(max(2048 // (N * ((Cc + 63) // 64)), 1), 64, P)
    return 2 * N * Cc * ch * 8 + N * 8 + N * Cc * 4 + 64


def test_the_workspaces_are_the_parents_and_hold_what_the_launchers_put_there(lib):
    for N, Cc, P in itertools.product((1, 2, 8, 33, 64), (1, 19, 256, 257, 4096), (1, 30, 63, 64, 65, 4097, 1 << 21)):
        ws = lib.ls_workspace(N, Cc, P)
        assert ws == parent_workspace(N, Cc, P)
        sel = call(lib, "ls_whmse", N, Cc, P)
        # the partials of every workgroup, then N weight sums, inside the workspace; the other families' partial arrays too
        assert sel["blocks"] * 8 <= sel["aux_off"] and sel["aux_off"] % 8 == 0 and sel["aux_off"] + 4 * N <= ws
        assert max(2 * L.MAX_BLOCKS, 3 * L.FOCAL_MAX_BLOCKS, 3 * L.MT_MAX_BLOCKS, 4 * L.MET_MAX_BLOCKS) * 8 <= sel["aux_off"]
        tws = lib.ls_topk_workspace(N, Cc, P)
        assert tws == parent_topk_workspace(N, Cc, P)
        c = dict(op="topk", shape=(N, Cc, 1, P), lay="cl", sdt="f32", tdt="f32", gdt="f32")
        tk = call(lib, "ls_topk", *three(c), 0, 2 * BASE, N, Cc, P)
        assert tk["aux_off"] == (2 * N * Cc * tk["chunks"] + N + N % 2) * 8 and tk["aux_off"] % 16 == 0 and tk["aux_off"] + 4 * N * Cc <= tws
    assert lib.ls_topk_workspace(0, 8, 8) == lib.ls_topk_workspace(8, 8, 0) == 64
