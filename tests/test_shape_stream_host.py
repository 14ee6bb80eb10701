"""Keeps tests/_shape_stream_cases.py honest without a GPU: every row's float64 reference runs, is finite and has the declared
shape; ids are unique; the two dispatch rules the table leans on (kd_small_linear's template choice, the small-wgrad block rule)
are restated in Python with their constants taken from csrc/gscnn_select.h, compiled for the host (tests/gscnn_select_host), and
the table is shown to hold a row on each side of them; the Canny line fixtures need more hysteresis rounds than the 8 x 64 sweeps
ops.canny used to stop at.  tests/test_gscnn_select_host.py holds the restatements themselves against the compiled selectors."""
import numpy as np
import pytest

import _shape_stream_cases as S
from test_gscnn_select_host import consts, load, sl_templates


@pytest.fixture(scope="module")
def lib():
    return load()


def test_case_ids_are_unique():
    ids = S.ids(S.CASES)
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("c", S.CASES, ids=S.ids(S.CASES))
def test_reference_runs_is_finite_and_has_the_declared_shape(c):
    inp, ref = S.build(c)
    shapes = S.expected_shapes(c)
    assert set(shapes) <= set(ref)
    for name, shape in shapes.items():
        assert tuple(ref[name].shape) == tuple(shape), f"{c['id']}: reference {name} has shape {tuple(ref[name].shape)}, declared {shape}"
        assert np.isfinite(np.asarray(ref[name], np.float64)).all()
        if c["op"] != "canny":
            assert ref[name].dtype == np.float64
    for name, a in inp.items():
        assert np.isfinite(a).all(), f"{c['id']}: input {name}"


def test_inputs_are_seeded():
    for c in (S.CASES[0], S.cases_of("gated_conv")[0], S.cases_of("canny")[-1]):
        a, b = S.build(c), S.build(c)
        for k in a[0]:
            assert np.array_equal(a[0][k], b[0][k])
        for k in a[1]:
            assert np.array_equal(a[1][k], b[1][k])


# ------------------------------------------------------------------------------------------------------ kd_small_linear
def test_small_linear_rows_sit_on_both_sides_of_every_template_boundary(lib):
    templates, maxc = sl_templates(lib), consts(lib)["SL_MAXC"]
    assert templates == S.SL_TEMPLATES and maxc == S.SL_MAXC == templates[-1], f"gscnn_select.h now lists {templates} (SL_MAXC {maxc}): retune the table"
    rows = S.cases_of("small_linear")
    couts = {c["cout"] for c in rows}
    for t in templates:
        assert t in couts and (t == maxc or t + 1 in couts), f"no row on both sides of Cout = {t}"
    assert 1 in couts
    forms = {"x_slice": lambda c: c["x_slice"] and c["x_dt"] == "bf16", "bias_relu": lambda c: c["bias"] and c["relu"],
             "acc_f32": lambda c: c["acc"] == "f32", "acc_bf16": lambda c: c["acc"] == "bf16", "mask": lambda c: c["mask"]}
    for t in templates:
        mine = [c for c in rows if S.sl_template(c["cout"], templates) == t]
        assert {c["cin"] for c in mine} >= {1, 33, 72}
        for name, has in forms.items():
            assert any(has(c) for c in mine), f"template {t}: no row with {name}"
    assert all(ci > maxc or co > maxc for ci, co in S.SL_REFUSED)


# ------------------------------------------------------------------------------------------------------- kd_small_wgrad
def test_small_wgrad_rows_reach_every_branch_of_the_block_rule(lib):
    K = consts(lib)
    k = dict(per_block=K["SW_PIX_PER_BLOCK"], max_blocks=K["SW_MAX_BLOCKS"], chunk=K["SW_CH"])
    assert k == dict(per_block=S.SW_PIX_PER_BLOCK, max_blocks=S.SW_MAX_BLOCKS, chunk=S.SW_CH), f"gscnn_select.h now has {k}: retune the table"
    assert K["THREADS"] == S.SW_THREADS
    rows = S.cases_of("small_wgrad")
    plan = {c["id"]: S.sw_blocks(c["npix"], **k) for c in rows}
    blocks = {nb for nb, _ in plan.values()}
    assert 1 in blocks and 2 in blocks and any(nb >= 3 for nb in blocks)
    for c in rows:
        nb, pb = plan[c["id"]]
        assert pb % k["chunk"] == 0 and (nb - 1) * pb < c["npix"] <= nb * pb
    last = lambda c: c["npix"] - (plan[c["id"]][0] - 1) * plan[c["id"]][1]      # pixels of the last block
    assert any(plan[c["id"]][0] == 1 and c["npix"] % k["chunk"] == 0 for c in rows), "no row of whole chunks only"
    assert any(plan[c["id"]][0] == 1 and c["npix"] > k["chunk"] and c["npix"] % k["chunk"] for c in rows), "no one-block row ending in a partial chunk"
    assert any(plan[c["id"]][0] >= 3 and last(c) % k["chunk"] for c in rows), "no row of three blocks whose last chunk is partial"
    assert any(c["npix"] < k["chunk"] for c in rows)
    assert any(c["ca"] * c["cb"] > S.SW_THREADS * 20 for c in rows), "no row that fills the last slot of the per-thread accumulator"
    assert any(c["ca"] * c["cb"] <= S.SW_THREADS for c in rows)
    # the table's own promises
    for n in (1479, 4097):
        assert {(c["ca"], c["cb"]) for c in rows if c["npix"] == n} >= set(S.SW_PAIRS)
    assert {c["npix"] for c in rows if (c["ca"], c["cb"]) == (33, 33)} >= set(S.SW_NPIX)
    assert {(c["a_dt"], c["b_dt"]) for c in rows} == {(a, b) for a in ("f32", "bf16") for b in ("f32", "bf16")}
    assert any(c["sliced"] for c in rows) and any(not c["bias"] for c in rows) and any(c["acc"] for c in rows)
    assert sum(c["twice"] for c in rows) == 1
    # the plan-only sizes: the block cap binds, and the round-up to whole chunks is what decides the number of blocks
    assert any(S.sw_blocks(n, **k)[0] == k["max_blocks"] for n in S.SW_PLAN_ONLY_NPIX)
    no_round_up = lambda n: -(-n // -(-n // min(max(-(-n // k["per_block"]), 1), k["max_blocks"])))
    assert any(S.sw_blocks(n, **k)[0] != no_round_up(n) for n in S.SW_PLAN_ONLY_NPIX)
    assert all(S.sw_blocks(c["npix"], **k)[0] == no_round_up(c["npix"]) for c in rows)     # (which is why data rows cannot see it)


# ------------------------------------------------------------------------------------------------------------ the others
def test_gated_conv_rows_cover_every_instantiation_and_pixel_group(lib):
    K = consts(lib)
    rows = S.cases_of("gated_conv")
    for C in (8, 16, 32):
        pix = lib.gs_gated_pix_of(C)
        assert pix == (K["GC_PIX_WIDE"] if C >= K["GC_WIDE_C"] else K["GC_PIX"]) and K["MFMA_PIX"] == 16
        for dt, kern in (("f32", "gated_conv_kernel"), ("bf16", "gated_conv_mfma_kernel")):
            n = {c["npix"] for c in rows if c["C"] == C and c["dt"] == dt and c["kernel"] == kern}
            assert any(v < pix for v in n) and any(v % pix for v in n if v > pix) and any(v % 16 == 0 for v in n) and any(v % 16 for v in n if v > 16)
    assert sorted(c["C"] for c in S.GC_VALU_BF16) == [8, 16, 32]
    # the parameter vector has the documented length
    for c in rows[:1] + S.GC_VALU_BF16:
        C = c["C"]
        assert S.build(c)[0]["params"].size == (C + 1) * (C + 1) + 2 * (C + 1) + 1 + C * C


def test_edge_aspp_reference_agrees_with_torch_interpolate():
    """The oracle's align-corners resample (the reference of the edge_aspp rows) against torch in float64 at every ratio of the
    table, Ho = 1 and H = 1 included."""
    import torch
    import torch.nn.functional as F
    from oracle import oracle as orc
    rng = np.random.default_rng(3)
    for hin, hout in S.EA_SIZES:
        a = rng.random((2, 1) + hin).astype(np.float32)
        ref = F.interpolate(torch.from_numpy(a).double(), size=hout, mode="bilinear", align_corners=True).numpy()
        assert np.abs(orc.upsample_bilinear_ac(a, hout) - ref).max() < 1e-6, (hin, hout)


def test_pointwise_small_output_stride_is_no_multiple_of_eight():
    for c in S.cases_of("pointwise_small"):
        ld = c["cout"] + S.PW_OUT_PAD
        assert ld % 4 == 0 and ld % 8 != 0 and S.PW_OUT_OFF % 4 == 0
    assert any(not c["bias"] for c in S.cases_of("pointwise_small"))


# ----------------------------------------------------------------------------------------------------------------- Canny
def test_canny_line_fixtures_need_more_rounds_than_the_old_sweep_budget():
    from oracle import oracle as orc
    by = {c["image"]: c for c in S.cases_of("canny") if c["image"] != "noise"}
    inp, ref = S.build(by["a"])
    img = inp["x"][0].transpose(1, 2, 0).astype(np.uint8)
    assert ref["edges"][0, 4].sum() == 1398 * 255 and (ref["edges"] > 0).sum() == 1403
    assert orc.canny_ref(img, S.CANNY_LOW, 10000).sum() == 0          # without the seed nothing is an edge: the line hangs on it
    assert ref["rounds"] > S.CANNY_OLD_BUDGET, ref["rounds"]
    inp_b, ref_b = S.build(by["b"])
    assert ref_b["rounds"] > S.CANNY_OLD_BUDGET and (ref_b["edges"] > 0).sum() > S.CANNY_OLD_BUDGET
    assert np.array_equal(inp_b["x"][0, 0], inp["x"][0, 0].T)
    inp_c, ref_c = S.build(by["c"])
    assert np.array_equal(ref_c["edges"][0, 4], ref["edges"][0, 4, ::-1])    # the mirrored line is the same edge
