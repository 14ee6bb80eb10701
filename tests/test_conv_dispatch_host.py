"""Keeps tests/_conv_dispatch_cases.py honest without a GPU: every KD_NOTE_KERNEL literal of the conv forward and weight-gradient
dispatchers is either the expected kernel of a table row or a name only an environment switch reaches; the pure-Python restatement
of both selections predicts every row's kernel; every gate has a row on each of its sides; and the restated workspace bound of the
ABI covers the restated launch plan, on the rows and over a sweep of shapes."""
import os
import re

import pytest

import _conv_dispatch_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "knowledge-distillation-by-replacing-cheap-conv_amd", "csrc")
SOURCES = ("conv_igemm.hip", "pw_wgrad.hip")


def note_arguments(text):
    """The argument text of every KD_NOTE_KERNEL(...) call (balanced parentheses, so ternaries over several lines are whole)."""
    out = []
    for m in re.finditer(r"KD_NOTE_KERNEL\s*\(", text):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        out.append(text[m.end():i - 1])
    return out


def declared_literals(sources=None):
    out = {}
    for name in SOURCES:
        if sources is None:
            with open(os.path.join(CSRC, name)) as f:
                text = f.read()
        else:
            text = sources[name]
        for arg in note_arguments(text):
            for lit in re.findall(r'"([^"]+)"', arg):
                out.setdefault(lit, name)
    return out


def coverage_gaps(declared, cases, switch_only):
    covered = {c["kernel"] for c in cases} | {n for c in cases for n in T.predict(c)["notes"]}
    msgs = []
    missing = sorted(set(declared) - covered - set(switch_only))
    if missing:
        msgs.append(f"kernel names no table row expects and SWITCH_ONLY does not list: {[(m, declared[m]) for m in missing]}")
    stale = sorted(set(switch_only) - set(declared))
    if stale:
        msgs.append(f"SWITCH_ONLY lists names the sources no longer declare: {stale}")
    both = sorted(set(switch_only) & covered)
    if both:
        msgs.append(f"names a default-environment row reaches are listed as switch-only: {both}")
    unknown = sorted(covered - set(declared))
    if unknown:
        msgs.append(f"rows expect names no source declares: {unknown}")
    return msgs


def gate_gaps(cases):
    have = {g for c in cases for g in c["gates"]}
    msgs = [f"gate {g!r} has no row on its side {s!r}" for g, sides in T.GATES.items() for s in sides if (g, s) not in have]
    msgs += [f"row marks an undeclared gate side {g!r}" for g in sorted(have) if g[0] not in T.GATES or g[1] not in T.GATES[g[0]]]
    return msgs


def test_every_noted_name_has_a_row_or_a_switch():
    declared = declared_literals()
    assert len(declared) >= 30, "the scan found too few KD_NOTE_KERNEL literals: has the macro been renamed?"
    assert not coverage_gaps(declared, T.CASES, T.SWITCH_ONLY), "\n".join(coverage_gaps(declared, T.CASES, T.SWITCH_ONLY))
    assert set(T.EPILOGUE_NOTES) <= set(declared)
    assert all(v.startswith("KDCC_") and "=" in v for v in T.SWITCH_ONLY.values())


def test_a_new_noted_name_and_a_stale_switch_name_are_reported():
    sources = {}
    for name in SOURCES:
        with open(os.path.join(CSRC, name)) as f:
            sources[name] = f.read()
    grown = dict(sources)
    grown["pw_wgrad.hip"] += '\nstatic void f(bool a) { KD_NOTE_KERNEL(a ? "new_kernel<a>"\n   : "new_kernel<b>"); }\n'
    msgs = coverage_gaps(declared_literals(grown), T.CASES, T.SWITCH_ONLY)
    assert len(msgs) == 1 and "new_kernel<a>" in msgs[0] and "new_kernel<b>" in msgs[0]
    msgs = coverage_gaps(declared_literals(), T.CASES, dict(T.SWITCH_ONLY, gone_kernel="KDCC_X=1"))
    assert len(msgs) == 1 and "gone_kernel" in msgs[0]


def test_every_gate_has_a_row_on_each_side():
    assert not gate_gaps(T.CASES), "\n".join(gate_gaps(T.CASES))


def test_deleting_the_only_row_on_a_side_is_reported():
    for victim in ("fwd:dil.rowx.65", "fwd:h.row.2dil-1", "wgrad:row.dil9", "pw:outside135"):
        rest = [c for c in T.CASES if c["id"] != victim]
        assert len(rest) == len(T.CASES) - 1
        assert gate_gaps(rest), f"dropping {victim} leaves no gap: its gate side has a second row, pick another victim"


def test_ids_and_reasons_are_unique_and_non_empty():
    ids, reasons = T.ids(T.CASES), [c["reason"] for c in T.CASES]
    assert all(ids) and len(set(ids)) == len(ids)
    assert all(r.strip() for r in reasons) and len(set(reasons)) == len(reasons)
    assert all(c["gates"] for c in T.CASES), "a row that sits on no gate"


@pytest.mark.parametrize("ncu", [256, 304, 64])
@pytest.mark.parametrize("c", T.CASES, ids=T.ids(T.CASES))
def test_the_restated_selection_predicts_the_row(c, ncu):
    """The expected name must not depend on the CU count; only the walk of the persistent grids may."""
    got = T.predict(c, ncu) if c["entry"] in ("conv2d", "conv2d_dgrad") else T.predict(c)
    assert got["kernel"] == c["kernel"], f"{c['id']}: the restated dispatcher picks {got['kernel']}, the row expects {c['kernel']}"
    if "tn_group" in c:
        assert got["tn_group"] == c["tn_group"]


def test_the_constants_the_restatement_uses_are_the_sources():
    """The tile types stay in conv_igemm.hip, which asserts conv_select.h's table against them; every gate expression is in
    conv_select.h, and in the whole library exactly once."""
    with open(os.path.join(CSRC, "conv_igemm.hip")) as f:
        conv = f.read()
    with open(os.path.join(CSRC, "pw_wgrad.hip")) as f:
        wg = f.read()
    with open(os.path.join(CSRC, "conv_select.h")) as f:
        sel = f.read()
    rows = dict(re.findall(r"typedef CfgRowT<8, 2, 4, 128, (\d+), 2, 2, 4, 1> (CfgRowX?);", conv))
    rows = {v: int(k) for k, v in rows.items()}
    assert (rows["CfgRow"] - 256) // 2 == T.ROW_MAXDIL and (rows["CfgRowX"] - 256) // 2 == T.ROWX_MAXDIL
    assert int(re.search(r"typedef CfgRowT<4, 4, 2, 64, (\d+), 3, 4> CfgRowN;", conv).group(1)) == 256 + 2 * T.ROWN_MAXDIL
    assert "MAXDIL = (AROWS - BM) / 2" in conv
    assert f"CONV_ROW_MAXDIL = {T.ROW_MAXDIL}, CONV_ROWX_MAXDIL = {T.ROWX_MAXDIL}, CONV_ROWN_MAXDIL = {T.ROWN_MAXDIL};" in sel
    assert "CfgRow::MAXDIL == CONV_ROW_MAXDIL && CfgRowX::MAXDIL == CONV_ROWX_MAXDIL && CfgRowN::MAXDIL == CONV_ROWN_MAXDIL" in conv
    assert "KD_REQUIRE(d->Cin % bk == 0" in conv and "const int bk = 128 / es;" in conv       # what makes REFUSED_CIN unreachable
    library = ""
    for name in sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".h", ".inc"))):
        with open(os.path.join(CSRC, name)) as f:
            library += f.read()
    for gate in (f"wide_tiles >= {T.WIDE_TILES_MIN}", "d->Cout > 128 &&", "d->W % 512 == 0 && d->dil <= 16 && d->Cin % 32 == 0", "d->H >= 2 * d->dil",
                 "d->Cin % 64 == 0 && d->H > d->dil", f"constexpr int WR_XROWS = {T.WR_XROWS};", "2 * d->dil + 64 <= WR_XROWS",
                 "d->Cout % 128 == 0 && d->dil <= 8", "pad256 * 100 <= pad128 * 135", f"< {T.WS_SPLIT_CAP} ? (stages + 7) / 8 : {T.WS_SPLIT_CAP}"):
        assert gate in sel and library.count(gate) == 1, gate
    assert "WR_XROWS" in wg                                                                    # the kernels' row buffer is the gate's constant


def test_grid_rows_walk_what_they_claim():
    for c in T.CASES:
        sides = dict(c["gates"])
        for g in ("fwd.grid.row", "fwd.grid.1x1", "fwd.grid.pp128"):
            if g not in sides:
                continue
            sel = T.fwd_select(c, 256)
            if sides[g] == "fewer":
                assert sel["ntiles"] < 256 and sel["grid"] == (sel["ntiles"] + 7) // 8 * 8
            else:
                assert all(sel["ntiles"] > n for n in (256, 264)), c["id"]
                assert sel["ntiles"] % 256 and sel["ntiles"] % 304, f"{c['id']}: the tile count divides a common CU count"


WG = T.cases_of("conv2d_wgrad", "pw_wgrad")


@pytest.mark.parametrize("c", WG, ids=T.ids(WG))
def test_restated_workspace_bound_covers_the_restated_plan(c):
    sel = T.wgrad_select(c)
    assert sel["need"] <= sel["workspace"], f"{c['id']}: the launch needs {sel['need']} bytes, the ABI's bound gives {sel['workspace']}"
    sides = dict(c["gates"])
    if sides.get("wgrad.plan.stages") in ("one", "one,row"):
        assert sel["stages"] == 1 and sel["splits"] == 1
    if sides.get("wgrad.plan.stages") == "under4":
        assert sel["stages"] < 4 and sel["splits"] == 1
    if sides.get("wgrad.plan.stages") == "under8,row":
        assert 1 < sel["stages"] < 8 and sel["splits"] == 1
    if sides.get("wgrad.plan.cap768") == "tr":
        assert sel["splits"] > T.WS_SPLIT_CAP
    if sides.get("wgrad.plan.cap768") == "wide":
        N, H, W = c["shape"][:3]
        assert (N * H * W // 64 + 7) // 8 == T.WS_SPLIT_CAP and sel["splits"] <= T.WS_SPLIT_CAP
    if "wgrad.reduce.n%4" in sides:
        assert sel["reduce4"] == (sides["wgrad.reduce.n%4"] == "on")


def test_restated_workspace_bound_over_a_sweep():
    """Every plan the dispatchers can take against the bound the ABI hands out (both restated): pixels from one stage to past the
    768-split cap, channels on both sides of every tile width, 1x1 and 3x3, both dtypes."""
    bad = []
    for M in (1, 63, 64, 65, 200, 512, 4096, 8 * 64 * 767 + 1, 8 * 64 * 768, 8 * 64 * 769, 8 * 64 * 1100, 1 << 21):
        for Cin in (8, 64, 128, 136, 248, 256, 304, 512, 1024):
            for Cout in (8, 19, 128, 136, 256, 304, 512):
                for k, W in ((1, 64), (3, 64), (3, 72)):
                    if M % W:
                        continue
                    for dt in ("bf16", "f32"):
                        for entry in ("conv2d_wgrad", "pw_wgrad"):
                            if entry == "pw_wgrad" and k != 1:
                                continue
                            c = dict(entry=entry, dt=dt, shape=(1, M // W, W, Cin, Cout, k, 1, k // 2, 1))
                            sel = T.wgrad_select(c)
                            if sel["need"] > sel["workspace"]:
                                bad.append((entry, dt, M, Cin, Cout, k, sel["splits"]))
    assert not bad, bad[:10]


def test_pairs_name_rows_that_exist():
    by_id = {c["id"]: c for c in T.CASES}
    for c in T.CASES:
        if "pair" in c:
            other, how = c["pair"]
            assert other in by_id and how in ("rows", "channels")
            assert by_id[other]["kernel"] != c["kernel"], f"{c['id']}: both sides of the pair run on the same kernel"
