"""Keeps tests/_nhwc_support_cases.py honest without a GPU: every KD_NOTE_PLUMBING literal of the BN / pool sources has a row and
every row names a declared literal; the trip counts a row claims follow from the launch plans restated there; the restated
workspace formulas are the built library's; rows sit on both sides of every gate; every reference runs and is finite with
finite, non-negative bounds (positive wherever the kernel computes); nothing has to be left out of a comparison."""
import os
import re

import numpy as np
import pytest

import _nhwc_support_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
SOURCES = ("hrnet_ops.hip", "bn_nhwc.hip", "dense_ops.hip", "bn_nhwc_core.h")


def declared_literals():
    out = {}
    for name in SOURCES:
        with open(os.path.join(CSRC, name)) as f:
            for lit in re.findall(r'KD_NOTE_PLUMBING\("([^"]+)"\)', f.read()):
                out.setdefault(lit, name)
    return out


def test_every_noted_literal_has_a_row_and_every_row_names_a_noted_literal():
    declared = declared_literals()
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
