"""Without a GPU: the rows of tests/test_scratch_gpu.py cover every kd_*_workspace export of include/kdcc.h, ops.py allocates scratch
at the seam only, and the poisoning allocator of tests/_scratch.py does what the GPU test relies on (on CPU tensors)."""
import ast
import importlib
import os
import re

import pytest
import torch

import _scratch as SC
import _scratch_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "knowledge-distillation-by-replacing-cheap-conv_amd")
SIZING = re.compile(r"kd_\w+_workspace")


def exports():
    with open(os.path.join(ROOT, "include", "kdcc.h")) as f:
        return set(re.findall(r"^size_t\s+(kd_\w+_workspace)\s*\(", f.read(), re.M))


def test_every_workspace_export_has_a_poison_row():
    """A new op that takes a workspace cannot land without a row that poisons it."""
    declared = exports()
    assert len(declared) >= 19 and "kd_loss_workspace" in declared and "kd_seg_jitter_workspace" in declared
    covered = T.sizing_covered()
    assert not declared - covered, f"no row of tests/_scratch_cases.py poisons the scratch of {sorted(declared - covered)}"
    assert not covered - declared, f"rows name sizing functions include/kdcc.h does not declare: {sorted(covered - declared)}"


def test_every_row_points_at_a_test_and_a_case_that_exist():
    assert len(set(T.ids())) == len(T.ROWS)
    defs = {}
    for r in T.ROWS:
        if r["module"] not in defs:
            with open(os.path.join(HERE, r["module"] + ".py")) as f:
                defs[r["module"]] = {n.name: n for n in ast.parse(f.read()).body if isinstance(n, ast.FunctionDef)}
        assert r["test"] in defs[r["module"]], f"{r['id']}: {r['module']}.py has no {r['test']}"
        params = [a.arg for a in defs[r["module"]][r["test"]].args.args]
        if r["table"] is not None:
            ids = [c["id"] for c in importlib.import_module(r["table"]).CASES]
            assert ids.count(r["case"]) == 1, f"{r['id']}: {r['table']} has {ids.count(r['case'])} rows with the id {r['case']}"
            assert "c" in params
        for p in params:
            assert p in ("K", "SEL", "c") or p in r["args"] or (p == "case" and "shape" in r["args"]), f"{r['id']}: nothing to pass {r['test']} as `{p}`"
    assert T.CRITERION_ROWS and all(r["module"] == "test_loss_dispatch_gpu" for r in T.CRITERION_ROWS)
    assert {s for r in T.CRITERION_ROWS for s in r["sizing"]} == {"kd_loss_workspace", "kd_topk_hint_workspace"}


def test_the_entry_points_a_row_records_exist_in_ops():
    with open(os.path.join(PKG, "ops.py")) as f:
        names = {n.name for n in ast.parse(f.read()).body if isinstance(n, ast.FunctionDef)}
    for r in T.ROWS:
        assert set(r["entries"]) <= names, f"{r['id']}: ops.py has no {sorted(set(r['entries']) - names)}"


def _calls(fn):
    for n in ast.walk(fn):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute):
            yield n


def _names(node):
    return {n.id for n in ast.walk(node) if isinstance(n, ast.Name)}


def handed_back(fn):
    """The names a function hands its caller: in a `return`, or appended to a list that is one of its parameters (conv2d's bn_sums)."""
    params = {a.arg for a in fn.args.args + fn.args.kwonlyargs}
    out = set()
    for n in ast.walk(fn):
        if isinstance(n, ast.Return) and n.value is not None:
            out |= _names(n.value)
        elif (isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "append" and isinstance(n.func.value, ast.Name)
              and n.func.value.id in params):
            out |= {x for a in n.args for x in _names(a)}
    return out


def bare_empties(fn):
    """Line numbers of the torch.empty calls of a function whose tensor is not a result: not assigned to names that are all handed back."""
    is_empty = lambda n: (isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "empty"
                          and isinstance(n.func.value, ast.Name) and n.func.value.id == "torch")
    results, ok = handed_back(fn), set()
    for st in ast.walk(fn):
        if isinstance(st, ast.Assign) and all(_names(t) and _names(t) <= results and not isinstance(t, (ast.Subscript, ast.Attribute)) for t in st.targets):
            ok |= {id(n) for n in ast.walk(st.value) if is_empty(n)}
    return sorted(n.lineno for n in ast.walk(fn) if is_empty(n) and id(n) not in ok)


def test_ops_allocates_scratch_at_the_seam_only():
    """No function of ops.py that sizes a workspace (names a kd_*_workspace function) calls torch.empty for anything but a result it
    hands back to its caller: its scratch comes from _ws / _scratch.  And the seam is there."""
    with open(os.path.join(PKG, "ops.py")) as f:
        tree = ast.parse(f.read())
    fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    assert {"_ws", "_scratch"} <= set(fns)
    sizing, bare = {}, []
    for name, fn in fns.items():
        sized = sorted({n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and SIZING.fullmatch(n.attr)})      # (called, or picked to be called)
        if not sized:
            continue
        sizing[name] = sized
        bare += [f"{name} (line {ln})" for ln in bare_empties(fn)]
        seam = [n.func.id for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)]
        assert {"_ws", "_bn_ws"} & set(seam) or name == "_bn_ws", f"{name} sizes {sized} and takes nothing from _ws"
    assert not bare, f"torch.empty for something that is not a returned result, next to a workspace sizing call (scratch goes through _ws / _scratch): {bare}"
    assert exports() == {s for v in sizing.values() for s in v}, "a kd_*_workspace export that no function of ops.py sizes with"


def test_the_seam_check_tells_scratch_from_results():
    """The rule above on the three shapes it has to tell apart."""
    src = (
        "def good(x, sums):\n"
        "    need = L.kd_x_workspace(1)\n"
        "    out = torch.empty(3)\n"
        "    a, b = torch.empty(1), torch.empty(2) if x else None\n"
        "    s12 = torch.empty(2)\n"
        "    sums.append((s12[0], s12[1]))\n"
        "    return out, a, b\n"
        "def bad(x, workspace=None):\n"
        "    need = L.kd_x_workspace(1)\n"
        "    if workspace is None:\n"
        "        workspace = torch.empty(need)\n"
        "    part = torch.empty(4)\n"
        "    f(torch.empty(5))\n"
        "    out = torch.empty(3)\n"
        "    return out\n")
    good, bad = ast.parse(src).body
    assert bare_empties(good) == [] and bare_empties(bad) == [11, 12, 13]


# ---------------------------------------------------------------------------------------------------- the allocator, on CPU tensors
@pytest.fixture
def ops():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    return ops


def stray(buf, offset, value=0x5A):
    """One byte stored `offset` bytes from the first byte of the handed-out buffer, through its own storage (as a kernel would)."""
    torch.as_strided(buf.view(torch.uint8).reshape(-1), (1,), (1,), buf.storage_offset() * buf.element_size() + offset).fill_(value)


@pytest.mark.parametrize("fill", SC.FILLS)
def test_poison_hands_out_the_filled_middle_of_a_guarded_allocation(ops, monkeypatch, fill):
    real = ops._ws, ops._scratch
    with SC.poison(monkeypatch, ops, fill, key="host", device="cpu") as p:
        a = ops._ws(100, "cpu")
        b = ops._ws(3, "cpu")                          # the floor of 16 bytes holds
        c = ops._ws(0, "cpu", 0)                       # ... and its absence
        s = ops._scratch((5, 2, 7), torch.float32, "cpu")
        h = ops._scratch((3, 8), torch.bfloat16, "cpu")
        assert (a.numel(), b.numel(), c.numel()) == (100, 16, 0) and a.dtype == torch.uint8
        assert tuple(s.shape) == (5, 2, 7) and s.dtype == torch.float32 and s.is_contiguous() and h.dtype == torch.bfloat16
        assert p.count == 5 and [x.nbytes for x in p.buffers] == [100, 16, 0, 280, 48]
        assert c.data_ptr() == 0                       # (an empty buffer is a null pointer to the library, as a bare torch.empty(0) is)
        for t, rec in zip((a, b, s, h), [x for x in p.buffers if x.nbytes]):
            # the pointer a kernel gets is as aligned as the allocation itself (the guard is a multiple of every alignment in use)
            assert t.data_ptr() - rec.whole.data_ptr() == SC.GUARD and SC.GUARD % 512 == 0
            assert t.data_ptr() % 64 == rec.whole.data_ptr() % 64
            assert rec.whole.numel() == rec.nbytes + 2 * SC.GUARD and rec.first_damage() is None and rec.high_water() == 0
        want = SC.fill_bytes(fill, 100 + 2 * SC.GUARD, "host:0")
        assert torch.equal(p.buffers[0].whole, want)
        if fill == "zero":
            assert not a.any() and not s.any()
        elif fill == "ones":
            assert bool(torch.isnan(s).all()) and bool(torch.isnan(h.float()).all()) and bool((a.view(torch.int32) == -1).all())
            assert bool(torch.isnan(ops._scratch((4,), torch.float64, "cpu")).all())
        else:
            assert len(set(p.buffers[0].whole.tolist())) > 100                       # bytes of every kind
            assert not torch.equal(p.buffers[0].whole[:200], p.buffers[3].whole[:200])      # another buffer, other bytes
            assert torch.equal(SC.fill_bytes("noise", 64, "k"), SC.fill_bytes("noise", 64, "k"))      # ... the same in every run
        a[10:20] = 7
        assert p.buffers[0].high_water() == 20
    assert (ops._ws, ops._scratch) == real, "the helpers were not put back"


@pytest.mark.parametrize("where", ("front-first", "front-last", "back-first", "back-last"))
@pytest.mark.parametrize("fill", SC.FILLS)
def test_one_byte_stored_in_a_guard_fails_the_block_and_names_the_buffer(ops, monkeypatch, fill, where):
    with pytest.raises(AssertionError) as e:
        with SC.poison(monkeypatch, ops, fill, key="host", device="cpu") as p:
            ops._ws(64, "cpu")
            buf = ops._bn_ws(100, 8, "cpu")            # an allocation made inside ops.py: the message names the function
            n = p.buffers[1].nbytes
            assert n == buf.numel() > 0
            at = {"front-first": -SC.GUARD, "front-last": -1, "back-first": n, "back-last": n + SC.GUARD - 1}[where]
            # (a stored byte that equals the fill cannot be seen, by any method: store another one)
            stray(buf, at, 0x5B if int(p.buffers[1].whole[SC.GUARD + at]) == 0x5A else 0x5A)
            buf[:] = 1                                  # the buffer itself is the kernel's to write
    side = "before the buffer" if at < 0 else f"{at - n} past its last byte"
    assert str(e.value).startswith(f"_bn_ws: scratch buffer 1 of {n} bytes ({fill} fill): the first changed guard byte is at offset {at} ({side})")


def test_a_write_inside_the_declared_bytes_is_no_damage(ops, monkeypatch):
    with SC.poison(monkeypatch, ops, "ones", device="cpu") as p:
        buf = ops._ws(100, "cpu")
        stray(buf, 0)
        stray(buf, 99)
    assert p.count == 1 and p.buffers[0].high_water() == 100


def test_the_criterion_caches_start_empty_or_seeded_and_are_put_back(ops, monkeypatch):
    mine, other = torch.zeros(8, dtype=torch.uint8), torch.ones(8, dtype=torch.uint8)
    monkeypatch.setitem(ops._ws_cache, "k", mine)
    monkeypatch.setitem(ops._topk_ws, "k", other)
    before = dict(ops._ws_cache), dict(ops._topk_ws)
    with SC.poison(monkeypatch, ops, "noise", device="cpu"):
        assert not ops._ws_cache and not ops._topk_ws
        ops._ws_cache["x"] = torch.zeros(1)
    assert (dict(ops._ws_cache), dict(ops._topk_ws)) == before and ops._ws_cache["k"] is mine and ops._topk_ws["k"] is other
    with SC.poison(monkeypatch, ops, "zero", seed_caches=1 << 12, device="cpu") as p:
        (k1, v1), = ops._ws_cache.items()
        (k2, v2), = ops._topk_ws.items()
        assert k1 == k2 == (torch.device("cpu"), 0) and v1.numel() == v2.numel() == 1 << 12 and v1.data_ptr() != v2.data_ptr()
        assert p.count == 2 and v1.data_ptr() == p.buffers[0].middle.data_ptr()
    assert (dict(ops._ws_cache), dict(ops._topk_ws)) == before
    with pytest.raises(RuntimeError, match="boom"):           # put back when the block raises, too
        with SC.poison(monkeypatch, ops, "zero", device="cpu"):
            ops._topk_ws["y"] = torch.zeros(1)
            raise RuntimeError("boom")
    assert (dict(ops._ws_cache), dict(ops._topk_ws)) == before
