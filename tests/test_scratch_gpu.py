"""No kernel depends on what its scratch memory held, and none writes past the bytes its kd_*_workspace() declared.

Every row of tests/_scratch_cases.py runs an existing GPU test on one row of its table three times, on identical inputs, with every
scratch buffer of ops.py (ops._ws / ops._scratch and the two criterion caches) handed out by the poisoning allocator of
tests/_scratch.py: pre-filled with 0x00, with 0xFF (NaN in every float format, -1 in every integer) and with seeded noise, between
two 4096-byte guards.  The existing test builds the row's inputs, asserts the kernel the table names and holds the result to the
table's reference and bound, unchanged, in each of the three runs; around it this file records the operands and results of the ops
entry points the row names and asserts that

  * the allocator handed out at least one buffer (a row that takes no scratch checks nothing),
  * every result is the same, bit for bit (integer views: NaN positions and signed zeros count), under the three fills,
  * every operand that is not a result is bitwise unchanged by the call,
  * every guard still holds its fill when the run ends (the first changed byte is named with the entry point that asked).

A kernel that reads a slot no block wrote, assumes a zeroed counter or stores one slot too far fails one of these whatever the
allocator happens to hold in production.  Two sequence tests run the criterion rows, in table order and reversed, through one shared
buffer in each criterion cache: what a larger call or another criterion left there must not reach the next result.

KDCC_SCRATCH_REPORT=path appends one JSON line per row (declared bytes and high-water mark of every buffer after the 0xFF run,
kernel reached, seconds): the source of profiles/scratch_poison.md.
"""
import importlib
import inspect
import json
import os
import sys
import time
import zlib

import numpy as np
import pytest
import torch

import _dw_dispatch_cases as D
import _scratch as SC
import _scratch_cases as T

pytestmark = pytest.mark.gpu

# the parameters of an entry point that it writes (results handed in by the caller); every other tensor operand must come back unchanged
RESULT_ARGS = {"out", "dw", "db", "dws", "dgamma", "dbeta", "running_mean", "running_var", "out_raw", "out_act", "cls_out", "bn_sums", "out_sums",
               "conf_s", "conf_t", "img", "grad"}
RESULT_ARGS_OF = {"bn_nhwc_stats": {"mean", "invstd", "var_unbiased"}}
# helpers of test_loss_dispatch_gpu.py that call the C interface themselves (a gradient view of the caller's): recorded like entry points
LOSS_HELPERS = ("two_operand_call", "ce_grad_call")
SEQUENCE_BYTES = 1 << 24        # the shared buffer of the sequence tests: no criterion row needs more (asserted there)


@pytest.fixture(scope="module")
def K():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    assert torch.cuda.is_available()
    return ops


def tensors(x):
    """Every tensor in a (nested) argument or return value; an ops.Lattice counts as its storage."""
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(getattr(x, "t", None), torch.Tensor):
        yield x.t
    elif isinstance(x, (list, tuple)):
        for e in x:
            yield from tensors(e)
    elif isinstance(x, dict):
        yield from tensors(list(x.values()))


def bits(t):
    """The bytes of a tensor's elements, on the host."""
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu() if t.numel() else torch.zeros(0, dtype=torch.uint8)


class Recorder:
    """Wraps entry points: keeps the bytes of every result of every call, and notes operands the call changed."""

    def __init__(self, marker=None):
        self.calls, self.damage = [], []
        self.marker, self.kernels = marker, []         # (report mode: the kernel names the recorded calls note, see Marker)

    def wrap(self, name, fn):
        sig = inspect.signature(fn)
        results = RESULT_ARGS | RESULT_ARGS_OF.get(name, set())

        def wrapped(*a, **kw):
            if isinstance(kw.get("workspace"), torch.Tensor):
                kw["workspace"] = None          # a buffer of the caller's own (the ABI's bound exactly): ops allocates as many bytes, at the seam
            args = sig.bind(*a, **kw).arguments
            written = {t.data_ptr() for n in results if n in args for t in tensors(args[n])}
            operands = [(n, t, t.clone()) for n, v in args.items() if n not in results for t in tensors(v) if t.data_ptr() not in written]
            if self.marker is not None:
                self.marker.leave()
            res = fn(*a, **kw)
            torch.cuda.synchronize()
            if self.marker is not None:
                self.kernels += [k for k in self.marker.noted() if k not in self.kernels]
            for n, t, before in operands:
                if not torch.equal(bits(t), bits(before)):
                    self.damage.append(f"{name}: operand `{n}` was written")
            self.calls.append((name, [bits(t) for t in tensors(res)] + [bits(t) for n in sorted(results) if n in args for t in tensors(args[n])]))
            return res
        return wrapped


class Marker:
    """Tells which kernel names an entry point notes (report mode only).  The library keeps the last name noted by the conv / depthwise
    dispatchers (_lib.last_kernel) and the last noted by the plumbing, BatchNorm, criterion and data entry points
    (_lib.last_plumbing_kernel), and has no way to clear either; an entry point that notes nothing leaves both as they were.  So a
    known name of another family is left in both slots before the call, and whatever stands there afterwards that is not the
    marker's was noted by the call."""

    def __init__(self, K):
        self.K = K
        self.x = torch.zeros((1, 4, 4, 16), device="cuda")
        self.taps = torch.zeros((9, 16), device="cuda")
        self.one = torch.ones(1, device="cuda")
        self.dwconv, self.scale = K.dwconv, K.scale_by_device_scalar_          # (the functions themselves: never a recorded wrapper)
        self.leave()
        self.names = self.slots()

    def slots(self):
        from kdcc_amd import _lib
        return _lib.last_kernel(), _lib.last_plumbing_kernel()

    def leave(self):
        self.dwconv(self.x, self.taps, 3, 1, 1)
        self.scale(torch.ones(8, device="cuda"), self.one)

    def noted(self):
        return [k for k, m in zip(self.slots(), self.names) if k != m]


def case_of(r):
    if r["table"] is None:
        return None
    hit = [c for c in importlib.import_module(r["table"]).CASES if c["id"] == r["case"]]
    assert len(hit) == 1, f"{r['id']}: {len(hit)} rows of {r['table']} have the id {r['case']}"
    return hit[0]


_FIXTURES = {}


def arguments(K, r, fn):
    """The test's parameters: its fixtures (K, and SEL of test_shape_stream_gpu.py), the table row as `c`, the row's own arguments."""
    kw = {}
    for name in inspect.signature(fn).parameters:
        if name == "K":
            kw[name] = K
        elif name == "SEL":
            if "SEL" not in _FIXTURES:
                _FIXTURES["SEL"] = importlib.import_module("test_gscnn_select_host").load()
            kw[name] = _FIXTURES["SEL"]
        elif name == "c":
            kw[name] = case_of(r)
        elif name == "case":
            kw[name] = r["args"]["shape"]
        else:
            kw[name] = r["args"][name]
    return kw


def memoized(fn, memo):
    def build(c):
        if c["id"] not in memo:
            memo[c["id"]] = fn(c)
        return memo[c["id"]]
    return build


def record(K, r, monkeypatch, memo, marker=None):
    """One run of the row's test with its entry points recorded -> (Recorder, the AssertionError the test raised or None)."""
    mod = sys.modules[__name__] if r["module"] == __name__ else importlib.import_module(r["module"])
    fn = getattr(mod, r["test"])
    rec, err = Recorder(marker), None
    with monkeypatch.context() as m:
        for e in r["entries"]:
            m.setattr(K, e, rec.wrap(e, getattr(K, e)))
        if r["module"] == "test_loss_dispatch_gpu":
            for h in LOSS_HELPERS:
                m.setattr(mod, h, rec.wrap(h, getattr(mod, h)))
        table = importlib.import_module(r["table"]) if r["table"] is not None else None
        if hasattr(table, "build"):     # the reference is computed once and shared by the three runs
            m.setattr(table, "build", memoized(table.build, memo))
        # (tests of test_ops_gpu.py draw from one module-wide generator: the same inputs in every run, and its own sequence left alone)
        m.setattr(importlib.import_module("test_ops_gpu"), "RNG", np.random.default_rng(zlib.crc32(r["id"].encode())))
        try:
            fn(**arguments(K, r, fn))
            torch.cuda.synchronize()
        except AssertionError as e:
            err = e
    return rec, err


def first_difference(r, base, calls, what):
    """None, or the message of the first result of `calls` that is not `base`'s bit for bit."""
    for i, (name, outs) in enumerate(base):
        if i >= len(calls):
            return None         # (the run ended early on an assertion of the test's own: raised by the caller)
        assert calls[i][0] == name and len(calls[i][1]) == len(outs), f"{r['id']}: call {i} is {calls[i][0]}, was {name}"
        for j, (a, b) in enumerate(zip(outs, calls[i][1])):
            if not torch.equal(a, b):
                at = int((a != b).nonzero()[0]) if a.shape == b.shape else -1
                return f"{r['id']}: result {j} of call {i} ({name}) differs {what}, first at byte {at} of {a.numel()}"
    return None


REPORT = os.environ.get("KDCC_SCRATCH_REPORT")


def report(K, r, p, monkeypatch, memo, seconds):
    """One line of the report, from inside the row's 0xFF run.  `kernel`: the name the row's table gives (the test asserts it after the
    launch); for a row of a table without names, the names an extra run sees its entry points note (Marker), "-" when they note none."""
    named = (case_of(r) or {}).get("kernel")
    buffers = [dict(entry=b.entry, declared=b.nbytes, high_water=b.high_water()) for b in p.buffers]
    entries = sorted({b.entry for b in p.buffers})
    if named:
        kernel, how = named, "table"
    else:
        kernel, how = " + ".join(record(K, r, monkeypatch, memo, Marker(K))[0].kernels) or "-", "observed"
    with open(REPORT, "a") as f:
        f.write(json.dumps(dict(id=r["id"], entries=entries, kernel=kernel, kernel_from=how, seconds=round(seconds, 3), buffers=buffers)) + "\n")


ISOLATED = {}       # row id -> the recorded calls of its run on zeroed scratch


@pytest.mark.parametrize("r", T.ROWS, ids=T.ids())
def test_results_do_not_depend_on_scratch_and_guards_hold(K, monkeypatch, r):
    memo, runs = {}, {}
    t0 = time.perf_counter()
    for fill in SC.FILLS:
        with SC.poison(monkeypatch, K, fill, key=r["id"]) as p:        # (leaving the block asserts the guards)
            rec, err = record(K, r, monkeypatch, memo)
            if fill == "ones" and REPORT:
                report(K, r, p, monkeypatch, memo, time.perf_counter() - t0)
        assert p.count >= 1 or err is not None, f"{r['id']}: the call took no scratch buffer: the row checks nothing"
        runs[fill] = (rec, err)
    base, base_err = runs["zero"]
    for fill in ("ones", "noise"):
        diff = first_difference(r, base.calls, runs[fill][0].calls, f"between the zero and the {fill} fill")
        assert diff is None, diff
    # the baseline itself is right: the table's reference, bound and kernel (asserted by the test, here re-raised) ...
    if base_err is not None:
        raise base_err
    assert base.calls, f"{r['id']}: none of {r['entries']} was called"
    for fill in ("ones", "noise"):          # ... and so is every poisoned run (the kernel the row claims, the same bound)
        if runs[fill][1] is not None:
            raise runs[fill][1]
        assert len(runs[fill][0].calls) == len(base.calls)
    for fill in SC.FILLS:
        assert not runs[fill][0].damage, f"{r['id']} ({fill} fill): {runs[fill][0].damage}"
    ISOLATED[r["id"]] = base.calls


def isolated(K, r, monkeypatch):
    if r["id"] not in ISOLATED:
        with SC.poison(monkeypatch, K, "zero", key=r["id"]):
            rec, err = record(K, r, monkeypatch, {})
        if err is not None:
            raise err
        ISOLATED[r["id"]] = rec.calls
    return ISOLATED[r["id"]]


@pytest.mark.parametrize("order", ("table-order", "reversed"))
def test_criteria_sharing_one_cache_buffer_equal_their_isolated_runs(K, monkeypatch, order):
    """Every criterion row through ONE buffer per cache, never refilled: a row finds what the rows before it left -- a larger call's
    partials behind its own, another criterion's counters -- and must return the loss and gradient of its isolated run on zeroed
    scratch, bit for bit."""
    seq = T.CRITERION_ROWS if order == "table-order" else T.CRITERION_ROWS[::-1]
    want = {r["id"]: isolated(K, r, monkeypatch) for r in seq}
    with SC.poison(monkeypatch, K, "zero", key="sequence", seed_caches=SEQUENCE_BYTES) as p:
        shared = [c[k].data_ptr() for c in (K._ws_cache, K._topk_ws) for k in c]
        assert len(shared) == 2
        for r in seq:
            rec, err = record(K, r, monkeypatch, {})
            diff = first_difference(r, want[r["id"]], rec.calls, f"from its isolated run when it follows the rows before it ({order})")
            assert diff is None, diff
            if err is not None:
                raise err
        assert [c[k].data_ptr() for c in (K._ws_cache, K._topk_ws) for k in c] == shared, "a row outgrew the shared buffer: the rows did not share it"
    assert p.count >= 2


# ------------------------------------------------------------------------------ rows whose launch no existing test makes in this form
def run_dwconv_wgrad(K, dt, shape):
    """The weight-gradient part of test_ops_gpu.test_dwconv_fwd_dgrad_wgrad (its inputs, oracle and bar), with accumulate=True after it
    as test_dwconv_wgrad_multi runs it."""
    import test_ops_gpu as TO
    N, H, W, Cc, k, p, d = shape
    x, gy = TO.q(TO.rnd(N, Cc, H, W), dt), TO.q(TO.rnd(N, Cc, H, W), dt)
    ref = TO.orc.conv2d_wgrad(x, gy, (Cc, 1, k, k), pad=p, dil=d, groups=Cc)
    xd, gd = TO.dev_nhwc(x, dt), TO.dev_nhwc(gy, dt)
    dw = torch.full((Cc, 1, k, k), 5.0, device="cuda")
    for acc in (False, True):
        K.dwconv_wgrad(xd, gd, dw, k, p, d, accumulate=acc)
        TO.selected(D.wgrad_kernel(dt, shape), f"dw wgrad {shape} {dt}")
        TO.assert_close(dw.cpu().numpy(), (2 if acc else 1) * ref, dt, f"dw wgrad{' accumulate' if acc else ''}")


def run_image_pool_from_sums(K):
    """aspp_image_pool(sums=) on the partial rows conv2d(out_sums=) hands it (`opart`): the conv of the dispatch table's fwd:out_sums row
    (test_conv_dispatch_gpu.run_forward checks it and its rows), then the pooling with and without the rows at the bars of
    test_ops_gpu.test_conv_output_sums_feed_the_image_pooling, whose own tensors are over 32 MiB."""
    import test_conv_dispatch_gpu as TC
    import test_ops_gpu as TO
    c = [c for c in TC.FWD if c["id"] == "fwd:out_sums"][0]
    seen, conv2d = {}, K.conv2d

    def spy(*a, **kw):
        res = conv2d(*a, **kw)
        seen.update(out=kw["out_raw"], sums=kw["out_sums"])
        return res
    with pytest.MonkeyPatch.context() as m:
        m.setattr(K, "conv2d", spy)
        TC.run_forward(K, c)
    out, sums = seen["out"], seen["sums"][0]
    N, H, W, Cout = out.shape
    red = 64
    wi = TO.rnd(red, Cout, scale=0.05)
    sc, sh = torch.from_numpy(TO.rnd(red) * 0.2 + 1.0).cuda(), torch.from_numpy(TO.rnd(red) * 0.1).cuda()
    a = torch.zeros((N, H, W, red), dtype=out.dtype, device="cuda")
    b = torch.zeros_like(a)
    K.aspp_image_pool(out, torch.from_numpy(wi).cuda(), sc, sh, a)
    K.aspp_image_pool(out, torch.from_numpy(wi).cuda(), sc, sh, b, sums=sums)
    assert float((a.float() - b.float()).abs().max()) <= 2.0 ** -7 * float(a.float().abs().max())
    mean = TO.host_nchw(out).mean(axis=(2, 3))
    want = np.maximum((mean @ wi.T) * sc.cpu().numpy() + sh.cpu().numpy(), 0)
    np.testing.assert_allclose(b.float().cpu().numpy()[:, 0, 0, :], want, rtol=2e-2, atol=2e-3)
    assert float((b.float() - b[:, :1, :1, :].float()).abs().max()) == 0.0
