"""Keeps tests/_plumbing_cases.py honest without a GPU: every name the three plumbing sources can note (the table of
csrc/plumb_select.h, compiled for the host) has a case, every case names one of them, the table is the set of literals the sources
noted before they had a table, every case's float64 reference runs and has the declared shape, the launch
plans the cases claim follow from the dispatcher's rules, and the large-offset channel really separates the kernel's
decomposition from a single fp32 chain where a case says so."""
import os
import re

import numpy as np
import pytest

import _plumbing_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
SOURCES = ("trunk_ops.hip", "bwd_ops.hip", "small_ops.hip")


# the KD_NOTE_PLUMBING("...") literals of the three sources as they stood before the names moved into plumb_select.h's table
# (recorded once with re.findall(r'KD_NOTE_PLUMBING\("([^"]+)"\)', source)): kd_debug_last_plumbing_kernel's vocabulary
PARENT_LITERALS = frozenset((
    "bn2d_bwd_kernel<eval>", "bn2d_bwd_kernel<train>", "bn2d_fwd_kernel<eval>", "bn2d_fwd_kernel<train>",
    "bn_eval_param_grads_kernel", "bn_fold_kernel", "bn_sums_stage_kernel<256 rows>", "bn_sums_stage_kernel<64 rows>",
    "broadcast_add_kernel<bf16>", "broadcast_add_kernel<f32>", "channel_sums_finish_kernel",
    "channel_sums_partial_kernel<bf16,1>", "channel_sums_partial_kernel<bf16,8>", "channel_sums_partial_kernel<f32,1>",
    "channel_sums_partial_kernel<f32,8>", "copy_cast_kernel<c_fast>", "copy_cast_kernel<p_fast>", "dconv_wgrad_kernel",
    "gap_partial_kernel<bf16>", "gap_partial_kernel<f32>", "maxpool_argmax_kernel<bf16>", "maxpool_argmax_kernel<f32>",
    "maxpool_bwd_kernel<bf16,1>", "maxpool_bwd_kernel<bf16,8>", "maxpool_bwd_kernel<f32,1>", "maxpool_bwd_kernel<f32,8>",
    "maxpool_kernel<bf16>", "maxpool_kernel<f32>", "relu_bn_bwd_kernel<bf16>", "relu_bn_bwd_kernel<f32>",
    "stem_conv_kernel<f32>", "stem_conv_mfma_kernel", "stem_pool_kernel", "stem_wgrad_kernel<bf16>", "stem_wgrad_kernel<f32>",
    "stem_wgrad_mfma_kernel", "upsample_bwd_kernel<bf16,bf16,1>", "upsample_bwd_kernel<bf16,bf16,8>",
    "upsample_bwd_kernel<bf16,f32,1>", "upsample_bwd_kernel<bf16,f32,8>", "upsample_bwd_kernel<f32,bf16,1>",
    "upsample_bwd_kernel<f32,bf16,8>", "upsample_bwd_kernel<f32,f32,1>", "upsample_bwd_kernel<f32,f32,8>",
    "upsample_flat4_kernel<bf16>", "upsample_flat4_kernel<f32>", "upsample_kernel<bf16,bf16,1>",
    "upsample_kernel<bf16,bf16,8>", "upsample_kernel<bf16,f32,1>", "upsample_kernel<bf16,f32,8>",
    "upsample_kernel<f32,bf16,1>", "upsample_kernel<f32,bf16,8>", "upsample_kernel<f32,f32,1>", "upsample_kernel<f32,f32,8>",
    "zero_insert_kernel<bf16>", "zero_insert_kernel<f32>"))


def declared_literals():
    """The names the launchers can note: the compiled table of csrc/plumb_select.h."""
    from test_plumb_select_host import load
    lib = load()
    return {lib.ps_name(k).decode(): "plumb_select.h" for k in range(lib.ps_refused())}


def test_every_noted_literal_has_a_case_and_every_case_names_a_noted_literal():
    declared = declared_literals()
    assert len(PARENT_LITERALS) == 56 and set(declared) == PARENT_LITERALS, sorted(set(declared) ^ PARENT_LITERALS)
    covered = {c["kernel"] for c in P.CASES}
    missing = sorted(set(declared) - covered)
    assert not missing, f"dispatch branches without a case in tests/_plumbing_cases.py: {[(m, declared[m]) for m in missing]}"
    unknown = sorted(covered - set(declared))
    assert not unknown, f"cases name kernels no source declares: {unknown}"


def test_every_note_goes_through_the_table():
    """No source notes a string literal any more: every KD_NOTE_PLUMBING takes plumb_kernel_name(sel.kernel)."""
    for name in SOURCES:
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        assert not re.search(r'KD_NOTE_PLUMBING\(\s*"', text), name
        notes = re.findall(r'KD_NOTE_PLUMBING\(([^;]*)\);', text)
        assert notes and set(notes) == {"plumb_kernel_name(sel.kernel)"}, (name, notes)


def test_the_conv_log_macro_is_untouched_in_the_plumbing_sources():
    """The KD_NOTE_KERNEL calls these files make stay as they are (bench.py and test_ddp_gpu.py read that log)."""
    seen = []
    for name in SOURCES:
        with open(os.path.join(CSRC, name)) as f:
            seen += re.findall(r'KD_NOTE_KERNEL\("([^"]+)"\)', f.read())
    assert sorted(seen) == ["stem_conv_kernel<f32>", "stem_conv_mfma_kernel", "stem_pool_kernel", "stem_wgrad_mfma_kernel"]


def test_case_ids_are_unique():
    ids = P.ids(P.CASES)
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("c", P.CASES, ids=P.ids(P.CASES))
def test_reference_runs_and_has_the_declared_shape(c):
    if c.get("big"):      # the 0.5-GB copy: the same row with a short plane runs the same reference path
        c = dict(c, shape=c["shape"][:3] + (1031,))
    inp, ref = P.build(c)
    for name, shape in P.expected_shapes(c).items():
        assert tuple(ref[name].shape) == tuple(shape), f"{c['id']}: reference {name} has shape {tuple(ref[name].shape)}, declared {shape}"
        if c["op"] != "copy_cast":
            assert np.isfinite(np.asarray(ref[name], dtype=np.float64)).all()


CS = P.cases_of("channel_sums")


@pytest.mark.parametrize("c", CS, ids=P.ids(CS))
def test_channel_sums_cases_reach_the_launch_plan_they_claim(c):
    N, H, W, C = c["shape"]
    groups, rows = (N, H * W) if c["per_image"] else (1, N * H * W)
    plan = P.cs_plan(groups, rows, C, c["vec"] == 8)
    for k, v in c.get("plan", {}).items():
        assert plan[k] == v, f"{c['id']}: {k} = {plan[k]}, the case claims {v}"
    if "ws_bytes" in c:
        assert groups * plan["cs_chunks"] * 2 * C * 4 == c["ws_bytes"]


@pytest.mark.parametrize("c", [c for c in P.CASES if "second_trip" in c], ids=lambda c: c["id"])
def test_grid_stride_cases_exceed_their_grid(c):
    work, cap_blocks = c["second_trip"]
    assert work > cap_blocks * 256


RED = P.cases_of(*P.REDUCTIONS)


def test_every_reduction_family_has_a_row_that_bites_or_says_why_not():
    for op in P.REDUCTIONS:
        rows = P.cases_of(op)
        assert all("chain" in c for c in rows), f"{op}: a row without its single-chain role"
        if not any(c["chain"][0] == "bites" for c in rows):
            assert op in ("bn2d_bwd", "stem_wgrad", "direct_wgrad"), f"{op}: no row separates the decomposition from a single chain"
    bf16 = [c for c in P.cases_of("channel_sums") if c["dt"] == "bf16" and c["chain"][0] == "bites"]
    assert bf16 and all(c["sub"] for c in bf16), "no bf16 row whose operands carry low bits"


@pytest.mark.parametrize("c", RED, ids=P.ids(RED))
def test_single_fp32_chain_against_the_bound(c):
    """For a row that says it bites, an fp32 sum of the same data in ONE chain must miss the bound the kernel's decomposition is
    held to, for every quantity the row names: the row then fails a kernel that loses the low bits.  For a row that says a
    single chain stays inside the bound, that is asserted too, so the table cannot claim more than the data give."""
    role, arg = c["chain"]
    inp, ref = P.build(c)
    got = P.single_chain(c, inp, ref)
    print({k: f"{e / max(b, 1e-300):.3g}" for k, (e, b) in got.items()})
    if role == "bites":
        for k in arg:
            err, bound = got[k]
            assert err > bound, f"{c['id']}: single-chain error of {k} {err:.3e} is inside the bound {bound:.3e}: the row proves nothing"
    elif role == "inside":
        assert isinstance(arg, str) and arg
        for k, (err, bound) in got.items():
            assert err <= bound, f"{c['id']}: single-chain error of {k} {err:.3e} exceeds the bound {bound:.3e}: the row bites, say so"
    else:
        assert role == "marginal" and isinstance(arg, str) and arg
