"""Keeps tests/_nhwc_support_cases.py honest without a GPU: every name the fp32 BN / pool launchers can note (the pool literals of
dense_ops.hip, the fp32 names of csrc/bn_select.h's compiled table) has a row and every row names one of them; the trip counts a
row claims follow from the launch plans restated there, and the restated float4 gate and grid are the compiled header's on the
rows' own values; the restated workspace formulas are the built library's; rows sit on both sides of every gate; every reference runs and is finite with
finite, non-negative bounds (positive wherever the kernel computes); nothing has to be left out of a comparison."""
import itertools
import os
import re

import numpy as np
import pytest

import _nhwc_support_cases as S
import _bn_select_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
SOURCES = ("hrnet_ops.hip", "bn_nhwc.hip", "dense_ops.hip", "bn_nhwc_core.h", "bn_select.h")


@pytest.fixture(scope="module")
def sel():
    return H.load()


def declared_literals(sel):
    """name -> where it is declared: the KD_NOTE_PLUMBING literals of the sources, and the fp32 names of the compiled bn_select.h
    table (what bn_nhwc_core.h and dense_ops.hip note through bn_kernel_name)."""
    out = {}
    for name in SOURCES:
        with open(os.path.join(CSRC, name)) as f:
            for lit in re.findall(r'KD_NOTE_PLUMBING\("([^"]+)"\)', f.read()):
                out.setdefault(lit, name)
    for k in range(sel.bl_count()):
        if sel.bl_name(k).decode().startswith("bn_nhwc_"):
            out.setdefault(sel.bl_name(k).decode(), "bn_select.h")
    return out


def test_every_noted_literal_has_a_row_and_every_row_names_a_noted_literal(sel):
    declared = declared_literals(sel)
    assert sorted(declared.values()).count("bn_select.h") == 5 and sorted(declared.values()).count("dense_ops.hip") == 4
    assert len(declared) == 9, f"expected the nine float4 / scalar / reduction-only choices, found {sorted(declared)}"
    assert "hrnet_ops.hip" not in declared.values(), "hrnet_ops.hip makes no host-side kernel choice"
    covered = {c["kernel"] for c in S.CASES if c["kernel"]}
    assert sorted(set(declared) - covered) == [], "dispatch branches without a row"
    assert sorted(covered - set(declared)) == [], "rows name kernels no source declares"
    for c in S.cases_of("bn_fwd", "bn_apply", "bn_bwd", "avgpool", "avgpool_bwd"):
        assert c["kernel"], f"{c['id']}: a row of a dispatching entry point without its kernel"


def test_row_ids_are_unique():
    assert len(S.ids(S.CASES)) == len(set(S.ids(S.CASES)))


def plan_of(c):
    op = c["op"]
    if op.startswith("ocr_"):
        return S.ocr_plan(c["shape"][1])
    V = int(c["kernel"][-2]) if c["kernel"] and c["kernel"].endswith(">") else 1
    if op.startswith("bn_"):
        return S.bn_plan(c["M"], c["C"], V)
    if op.startswith("avgpool"):
        N, H, W, C = c["shape"]
        return S.pool_plan(N * (H // 2) * (W // 2) if op == "avgpool" else N * H * W, C, V)
    return {}


PLANNED = [c for c in S.CASES if c["plan"]]


@pytest.mark.parametrize("c", PLANNED, ids=S.ids(PLANNED))
def test_rows_reach_the_trip_counts_they_claim(c):
    plan = plan_of(c)
    for k, v in c["plan"].items():
        assert plan[k] == v, f"{c['id']}: {k} = {plan[k]}, the row claims {v}"


def test_kernel_choice_follows_vec4_ok_alone():
    """The three ways out of the float4 path, each alone, on every operand alone; an unread y and aligned slices stay on it."""
    assert not S.vec4_ok(6, []) and not S.vec4_ok(8, [(0, 10)]) and not S.vec4_ok(8, [(2, 12)]) and S.vec4_ok(8, [(4, 16), None, (8, 24)])
    by_id = {c["id"]: c for c in S.CASES}
    for name in ("ld10", "off2"):
        for who in ("x", "y"):
            c = by_id[f"bn_apply:{name}-on-{who}"]
            assert c["kernel"] == "bn_nhwc_apply_kernel<1>" and list(c["views"]) == [who] and c["C"] % 4 == 0
        for who in ("gy", "x", "y", "res", "dx"):
            c = by_id[f"bn_bwd:{name}-on-{who}"]
            assert c["kernel"] == "bn_nhwc_dx_kernel<1>" and list(c["views"]) == [who] and c["relu"] and c["flags"]["res"]
        assert by_id[f"bn_bwd:{name}-on-unread-y"]["kernel"] == "bn_nhwc_dx_kernel<4>" and not by_id[f"bn_bwd:{name}-on-unread-y"]["relu"]
        for op, ab in (("avgpool", ("x", "y")), ("avgpool_bwd", ("gy", "gx"))):
            for who in ab:
                c = by_id[f"{op}:{name}-on-{who}"]
                assert c["kernel"].endswith("<1>") and list(c["views"]) == [who]
    for cid in ("bn_apply:aligned-slices", "bn_bwd:aligned-slices", "avgpool:aligned-slices", "avgpool_bwd:aligned-slices"):
        assert by_id[cid]["kernel"].endswith("<4>") and by_id[cid]["views"]
    assert by_id["bn_apply:C6"]["kernel"].endswith("<1>") and by_id["bn_bwd:C6-res"]["kernel"].endswith("<1>")
    assert by_id["bn_bwd:no-dx-dgamma-only"]["kernel"] == "bn_nhwc_grad_finish_kernel"


def test_the_restated_gate_and_grid_are_the_compiled_headers(sel):
    """S.vec4_ok / S.grid_for / S.bn_plan (the independent model the rows' kernels and trip counts come from) against csrc/bn_select.h
    compiled for the host with es = 4, over the rows' own C, float offsets and leading dimensions: one view at a time off the
    dense layout, on every operand of the forward, the backward and the two-view (pool) gate, and every row's own views."""
    Cs = sorted({c["C"] for c in S.CASES if "C" in c} | {c["shape"][3] for c in S.cases_of("avgpool", "avgpool_bwd")})
    views = sorted({v for c in S.CASES if c["op"].startswith(("bn_", "avgpool")) for v in c["views"].values()} | {(0, 0)})
    Ms = sorted({c["M"] for c in S.CASES if "M" in c})
    assert {6, 8, 512, 129} <= set(Cs) and {(0, 10), (2, 12), (4, 16)} <= set(views) and {1, 2049, 16400} <= set(Ms)
    ptr = lambda C, v: (H.BASE + 4 * v[0], v[1] or C)
    for C, v in itertools.product(Cs, views):
        if v[1] and v[1] < C:
            continue
        odd, base = ptr(C, v), (H.BASE, C)
        mv = (v[0], v[1] or C)
        for who in range(2):
            a = [base, base]
            a[who] = odd
            want = S.vec4_ok(C, [mv if i == who else (0, C) for i in range(2)])
            assert bool(sel.bl_vec_ok(4, C, *a[0], *a[1])) == want, (C, v, who)
            got = H.call(sel, "fwd", 4, *a[0], *a[1], 129, C)
            assert (got["vec"], got["part_vec"]) == (want, 0) and got["name"] == f"bn_nhwc_apply_kernel<{4 if want else 1}>"
        for who, name in enumerate(H.OPERANDS):
            for present in itertools.product((False, True), repeat=3):      # y (relu), res, dx
                there = dict(zip(("y", "res", "dx"), present), gy=True, x=True)
                ops = {n: (odd if n == name else base) for n in H.OPERANDS if there[n]}
                want = S.vec4_ok(C, [None if not there[n] else (mv if n == name else (0, C)) for n in H.OPERANDS])
                got = H.bwd(sel, 4, 129, C, ops)
                kern = f"bn_nhwc_dx_kernel<{4 if want else 1}>" if there["dx"] else "bn_nhwc_grad_finish_kernel"
                assert (got["vec"], got["part_vec"], got["name"]) == (want, 0, kern), (C, v, name, present)
    for M, C, V in itertools.product(Ms, Cs, (1, 4)):
        if C % V:
            continue
        p = S.bn_plan(M, C, V)
        ld = C if V == 4 else C + 1         # a leading dimension of C + 1 is never on the float4 path
        for got, ch in ((H.call(sel, "fwd", 4, H.BASE, ld, H.BASE, ld, M, C), 16), (H.bwd(sel, 4, M, C, {n: (H.BASE, ld) for n in H.OPERANDS}), 64)):
            assert got["vec"] == (V == 4) and (got["nrb"], got["grid"]) == (p["nrb"], p["grid"]) == (S.nrb(M), S.grid_for(M * (C // V))), (M, C, V)
            assert (got["part_x"], got["part_y"], got["finish"]) == (S.nrb(M), -(-C // 64), -(-C // ch))
    for t in (-5, 0, 1, 256, 257, 8192 * 256 - 1, 8192 * 256, 8192 * 256 + 1, 1 << 40):
        assert sel.bl_grid(t) == S.grid_for(t), t
    # every dispatching row: the kernel the table gives it is what the compiled selector (pools: the compiled two-view gate) answers
    for c in S.cases_of("bn_fwd", "bn_apply", "bn_bwd", "avgpool", "avgpool_bwd"):
        C = c["C"] if "C" in c else c["shape"][3]
        at = lambda n: ptr(C, c["views"].get(n, (0, 0)))
        if c["op"] == "bn_bwd":
            names = ["gy", "x"] + (["y"] if c["relu"] else []) + (["res"] if c["flags"].get("res") else []) + (["dx"] if c["flags"].get("need_dx", True) else [])
            assert H.bwd(sel, 4, c["M"], C, {n: at(n) for n in names})["name"] == c["kernel"], c["id"]
        elif c["op"].startswith("bn_"):
            assert H.call(sel, "fwd", 4, *at("x"), *at("y"), c["M"], C)["name"] == c["kernel"], c["id"]
        else:
            a, b = ("x", "y") if c["op"] == "avgpool" else ("gy", "gx")
            assert int(c["kernel"][-2]) == (4 if sel.bl_vec_ok(4, C, *at(a), *at(b)) else 1), c["id"]


def test_bn_shapes_cover_both_sides_of_every_flag():
    assert {m for m, _, _, _ in S.BN_SHAPES} == {1, 127, 128, 129, 384, 513, 2048, 2049}
    for C in (1, 3, 4, 6, 17, 65, 68):
        rows = [s for s in S.BN_SHAPES if s[1] == C]
        assert {t for _, _, t, _ in rows} == {True, False} and {r for _, _, _, r in rows} == {True, False}, f"C = {C}"
    res_rows = [c for c in S.cases_of("bn_bwd") if c["flags"].get("res")]
    assert {c["kernel"] for c in res_rows} == {"bn_nhwc_dx_kernel<4>", "bn_nhwc_dx_kernel<1>"}


def test_big_rows_exceed_the_grid_cap_per_kernel_and_V():
    big = [c for c in S.CASES if c["flags"].get("big")]
    assert sorted(c["kernel"] for c in big) == sorted(
        [f"{k}<{v}>" for k in ("bn_nhwc_apply_kernel", "bn_nhwc_dx_kernel", "avgpool2x2_kernel", "avgpool2x2_bwd_kernel") for v in (1, 4)])
    for c in big:
        p = plan_of(c)
        assert p["grid"] == 8192 and p["trips"] == 2, c["id"]
        assert plan_of(S.shorten(c))["trips"] == 1


def test_rows_sit_on_both_sides_of_every_gate():
    hw = {c["shape"][1] for c in S.cases_of("ocr_gather")}
    hw_bwd = {c["shape"][1] for c in S.cases_of("ocr_gather_bwd")}
    for lo, hi, key in ((64, 65, "chunks"), (2048, 2113, "tiles"), (8192, 8257, "stats_trips")):
        assert {lo, hi} <= hw and S.ocr_plan(lo)[key] == 1 and S.ocr_plan(hi)[key] == 2, (lo, hi, key)
    assert {1024, 1025} <= hw_bwd and S.ocr_plan(1024)["bwd_trips"] == 1 and S.ocr_plan(1025)["bwd_trips"] == 2
    assert {2113} <= {c["shape"][1] for c in S.cases_of("ocr_attend_bwd")}
    ms = {c["M"] for c in S.cases_of("bn_fwd", "bn_stats") if c["train"]}
    assert {2048, 2049} <= ms and S.bn_plan(2048, 4, 1)["finish_trips"] == 1 and S.bn_plan(2049, 4, 1)["finish_trips"] == 2
    assert any(S.nrb(c["M"]) < 4 for c in S.cases_of("bn_bwd")) and S.nrb(2048) == 16 and S.nrb(2049) == 17
    # the LDS limits at equality and one channel step over
    gb = {c["shape"][2:] for c in S.cases_of("ocr_gather_bwd")}
    at = {c["shape"][2:] for c in S.cases_of("ocr_attend")}
    refused = {(op, s[2:]) for op, s in S.REFUSALS}
    assert (32, 512) in gb and 32 * 512 * 4 == S.OCR_LDS_LIMIT and ("ocr_gather_bwd", (32, 516)) in refused and not S.gather_bwd_lds_ok(32, 516)
    assert (32, 516) not in gb and S.gather_bwd_lds_ok(32, 512)
    assert (32, 256) in at and 2 * 32 * 256 * 4 == S.OCR_LDS_LIMIT and ("ocr_attend", (32, 260)) in refused and not S.attend_lds_ok(32, 260)
    assert (19, 428) in at and S.attend_lds_ok(19, 428) and ("ocr_attend", (19, 432)) in refused and not S.attend_lds_ok(19, 432)


def test_restated_workspaces_are_the_librarys():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import _lib
    L = _lib.lib()
    for c in S.CASES:
        if c["op"].startswith("ocr_gather"):
            assert L.kd_ocr_gather_workspace(*c["shape"]) == S.ocr_gather_workspace(*c["shape"]), c["id"]
        elif c["op"].startswith("ocr_attend"):
            assert L.kd_ocr_attend_workspace(*c["shape"]) == S.ocr_attend_workspace(*c["shape"]), c["id"]
        elif c["op"].startswith("bn_"):
            assert L.kd_bn_nhwc_workspace(c["M"], c["C"]) == S.bn_workspace(c["M"], c["C"]), c["id"]
    for op, shape in S.REFUSALS:
        ws = L.kd_ocr_gather_workspace if op.startswith("ocr_gather") else L.kd_ocr_attend_workspace
        assert ws(*shape) == (S.ocr_gather_workspace if op.startswith("ocr_gather") else S.ocr_attend_workspace)(*shape)


def test_ocr_maxima_sit_where_the_rows_say():
    for c in S.cases_of("ocr_gather"):
        inp, ref = S.build(c)
        N, HW, K, C = c["shape"]
        per, cnt = S.ocr_chunks(HW)
        assert (inp["logits"][:, :, 0].argmax(1) == HW - 1).all(), c["id"]
        if cnt > 1 and K > 1:
            assert (inp["logits"][:, :, 1].argmax(1) == per).all(), c["id"]
        if c["flags"].get("spread"):
            assert np.ptp(inp["logits"]) > 55


@pytest.mark.parametrize("c", S.CASES, ids=S.ids(S.CASES))
def test_reference_runs_with_finite_bounds_and_leaves_nothing_out(c):
    c = S.shorten(c)
    inp, ref = S.build(c)
    got = S.checks(c, ref)
    assert got, f"{c['id']}: no output to compare"
    for name, r, b in got:
        r = np.asarray(r, dtype=np.float64)
        b = np.asarray(b, dtype=np.float64) + np.zeros_like(r)
        assert r.shape == b.shape and np.isfinite(r).all() and np.isfinite(b).all() and (b >= 0).all(), f"{c['id']} {name}"
        if S.is_exact(c, name):
            assert not b.any(), f"{c['id']} {name}: a moved value is compared bit for bit"
        else:
            assert (b[r != 0] > 0).all(), f"{c['id']} {name}: a computed value with a zero bound"
            assert b.max() <= 1e-2 * max(np.abs(r).max(), 1.0), f"{c['id']} {name}: a bound of the order of the value decides nothing"
    assert S.sign_agrees(c, inp, ref) <= S.LEFT_OUT_CAP
    if c["op"] in ("hr_fuse_bwd", "bn_bwd") and c.get("relu", True):
        assert 0.05 < float(np.mean(inp["y"] > 0)) < 0.95 or inp["y"].size < 64, f"{c['id']}: the ReLU mask is one-sided"
