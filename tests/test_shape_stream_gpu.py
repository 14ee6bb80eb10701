"""Every branch of the Gated-SCNN shape-stream kernels (csrc/gscnn_ops.hip, csrc/gscnn_bwd.hip) against float64 references of
the module expressions on the operands as stored (tests/_shape_stream_cases.py).

Acceptance is per element: test_ops_gpu.assert_close (max error over the reference's range 1e-3 for fp32 storage, 1.5e-2 for
bf16 storage, plus its relative-L2 bound), by the storage type of the OUTPUT: the references see the operands already rounded
to their storage type, so a kernel with fp32 arithmetic and an fp32 output is held to the fp32 bar whatever its operands are
stored as.  fp32 kd_small_wgrad keeps the 1e-4 norm bar of test_gscnn_gpu.py as well.  Every case that writes a channel slice
fills the buffer with 7.0 first and asserts the rest untouched.  Canny is bit for bit.  Every row also asserts the kernel it reached
(kd_debug_last_plumbing_kernel) against what csrc/gscnn_select.h, compiled for the host, selects for the row's call; a refused
call leaves that slot and its output alone.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import _shape_stream_cases as S
from _shape_stream_child import run_gated_conv
from test_gscnn_select_host import REFUSED, call, load, select
from test_ops_gpu import assert_close

pytestmark = pytest.mark.gpu

DT = S.DT


@pytest.fixture(scope="module")
def K():
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope="module")
def SEL():
    return load()


def reached(SEL, c, sel=None):
    """The call the row just made noted the kernel the compiled selector names for it (and the row claims)."""
    from kdcc_amd import _lib
    want = (sel or select(SEL, c))["name"]
    got = _lib.last_plumbing_kernel()
    assert got == want, f"{c['id']}: the launch went to {got}, gscnn_select.h selects {want}"
    if sel is None:
        assert want == S.slot_name(c), f"{c['id']}: this row is meant to cover {S.slot_name(c)}"


def other_family_marker(K):
    """Leaves a name of another entry point in the slot (the one-pixel edge_attention row) and returns it."""
    from kdcc_amd import _lib
    c = S.cases_of("edge_attention")[0]
    inp, _ = S.build(c)
    K.edge_attention(cs_view(inp, c["dt"]), dev(inp["canny"]), dev(inp["w"]))
    assert _lib.last_plumbing_kernel() == c["kernel"]
    return c["kernel"]


def dev(a, dt="f32"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DT[dt]).cuda()


def view(a, dt, sliced, off=8, pad=16, fill=7.0):
    """(view holding `a`, whole buffer): a channel slice at element `off` of a buffer `pad` channels wider, or dense."""
    t = dev(a, dt)
    if not sliced:
        return t, t
    C = t.shape[-1]
    buf = torch.full(tuple(t.shape[:-1]) + (C + pad,), fill, dtype=t.dtype, device="cuda")
    buf[..., off:off + C] = t
    return buf[..., off:off + C], buf


def untouched(v, buf, off=8):
    if v is buf:
        return
    C = v.shape[-1]
    assert bool((buf[..., :off] == 7.0).all()) and bool((buf[..., off + C:] == 7.0).all()), "wrote outside the channel slice"


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def rel_norm(got, ref):
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


# ---------------------------------------------------------------------------------------------------------- kd_small_linear
SL = S.cases_of("small_linear")


@pytest.mark.parametrize("c", SL, ids=S.ids(SL))
def test_small_linear(K, SEL, c):
    inp, ref = S.build(c)
    x, _ = view(inp["x"], c["x_dt"], c["x_slice"])
    kw = dict(relu=c["relu"], bias=dev(inp["bias"]) if c["bias"] else None)
    if c["mask"]:
        kw["mask"], _ = view(inp["mask"], "f32", True)
    if c["acc"]:
        out, buf = view(inp["y0"], c["acc"], True)
        K.small_linear(x, dev(inp["w"]), out=out, accumulate=True, **kw)
        untouched(out, buf)
        odt = c["acc"]
    else:
        out = K.small_linear(x, dev(inp["w"]), out_dtype=torch.float32, **kw)
        odt = "f32"
    reached(SEL, c)
    assert tuple(out.shape) == (S.SL_PIX, c["cout"])
    assert_close(host(out), ref["y"], odt, c["id"])


@pytest.mark.parametrize("cin,cout", S.SL_REFUSED)
def test_small_linear_refuses_more_than_72_channels(K, SEL, cin, cout):
    from kdcc_amd import _lib
    x, w = torch.zeros((4, cin), device="cuda"), torch.zeros((cout, cin), device="cuda")
    out = torch.full((4, cout), 7.0, device="cuda")
    assert call(SEL, "small_linear", 0, cin, cin, 0, cout, cout, 4, 0, 0)["name"] == REFUSED
    marker = other_family_marker(K)
    with pytest.raises(_lib.KdccError):
        K.small_linear(x, w, out=out)
    assert _lib.last_plumbing_kernel() == marker and bool((out == 7.0).all()), "a refused call launched something"


# ----------------------------------------------------------------------------------------------------------- kd_small_wgrad
SW = S.cases_of("small_wgrad")


@pytest.mark.parametrize("c", SW, ids=S.ids(SW))
def test_small_wgrad(K, SEL, c):
    inp, ref = S.build(c)
    a, _ = view(inp["a"], c["a_dt"], c["sliced"])
    b, _ = view(inp["b"], c["b_dt"], c["sliced"])

    def run():
        kw = {}
        if c["acc"]:
            kw = dict(dw=dev(inp["dw0"]), db=dev(inp["db0"]) if c["bias"] else None, accumulate=True)
        return K.small_wgrad(a, b, want_bias=c["bias"], **kw)
    dw, db = run()
    reached(SEL, c)
    assert tuple(dw.shape) == (c["cb"], c["ca"]) and dw.dtype == torch.float32
    both_f32 = c["a_dt"] == c["b_dt"] == "f32"
    for name, got in (("dw", dw), ("db", db)):
        if name == "db" and not c["bias"]:
            assert got is None
            continue
        g = host(got)
        print(f"{c['id']} {name}: rel norm {rel_norm(g, ref[name]):.3e}")
        assert_close(g, ref[name], "f32", f"{c['id']} {name}")
        if both_f32:
            assert rel_norm(g, ref[name]) < 1e-4, f"{c['id']} {name}"
    if c["twice"]:
        dw2, db2 = run()
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "two identical calls differ: the reduction order is not fixed"


@pytest.mark.parametrize("npix", sorted({c["npix"] for c in SW}) + S.SW_PLAN_ONLY_NPIX)
def test_small_wgrad_workspace_follows_the_block_rule(K, npix):
    """kd_small_wgrad_workspace is one partial per block: the block count of the small-wgrad rule (restated in the table, held to the
    compiled header by test_gscnn_select_host.py) at every pixel count of the table and where the 1024-block cap binds."""
    from kdcc_amd import _lib
    for ca, cb in ((33, 33), (72, 1)):
        assert _lib.lib().kd_small_wgrad_workspace(ca, cb, npix) == S.sw_workspace(ca, cb, npix), (ca, cb, npix, S.sw_blocks(npix))


# ---------------------------------------------------------------------------------------------------------- kd_gate_mix_bwd
GM = S.cases_of("gate_mix_bwd")


@pytest.mark.parametrize("c", GM, ids=S.ids(GM))
def test_gate_mix_bwd(K, SEL, c):
    inp, ref = S.build(c)
    feat, _ = view(inp["feat"], c["dt"], True)
    gv = dev(inp["gv"]) if "gv" in inp else None
    gfeat, ga, v = K.gate_mix_bwd(feat, dev(inp["a"]), gv=gv, want_v=c["outs"] != "grads-only")
    reached(SEL, c)
    got = {"gfeat": gfeat, "ga": ga, "v": v}
    for name in ("gfeat", "ga", "v"):
        if name in ref:
            assert tuple(got[name].shape) == tuple(ref[name].shape)
            assert_close(host(got[name]), ref[name], "f32", f"{c['id']} {name}")
        else:
            assert got[name] is None


# ---------------------------------------------------------------------------------------- kd_edge_attention (+ its backward)
def cs_view(inp, dt):
    buf = torch.full(inp["cs"].shape[:-1] + (64,), 7.0, dtype=DT[dt], device="cuda")      # the first 8 channels of 64
    buf[..., :8] = dev(inp["cs"], dt)
    return buf


EA = S.cases_of("edge_attention")


@pytest.mark.parametrize("c", EA, ids=S.ids(EA))
def test_edge_attention(K, SEL, c):
    inp, ref = S.build(c)
    acts = K.edge_attention(cs_view(inp, c["dt"]), dev(inp["canny"]), dev(inp["w"]))
    reached(SEL, c)
    assert tuple(acts.shape) == tuple(ref["acts"].shape) and acts.dtype == torch.float32
    assert_close(host(acts), ref["acts"], "f32", c["id"])


EB = S.cases_of("edge_attention_bwd")


@pytest.mark.parametrize("c", EB, ids=S.ids(EB))
def test_edge_attention_bwd(K, SEL, c):
    inp, ref = S.build(c)
    g_t, g_s, eoc = K.edge_attention_bwd(cs_view(inp, c["dt"]), dev(inp["canny"]), dev(inp["w"]), dev(inp["g"]))
    reached(SEL, c)
    assert tuple(eoc.shape) == tuple(ref["eo"].shape) + (2,)
    assert_close(host(g_t), ref["g_t"], "f32", f"{c['id']} g_t")
    assert_close(host(g_s), ref["g_s"], "f32", f"{c['id']} g_s")
    assert_close(host(eoc[..., 0]), ref["eo"], "f32", f"{c['id']} eo_canny[:, 0]")
    assert np.array_equal(host(eoc[..., 1]), ref["canny"]), f"{c['id']} eo_canny[:, 1]"      # a copy of the 0 / 255 map


# ----------------------------------------------------------------------------------------------------------------- kd_edge_aspp
EP = S.cases_of("edge_aspp")


@pytest.mark.parametrize("c", EP, ids=S.ids(EP))
def test_edge_aspp(K, SEL, c):
    inp, ref = S.build(c)
    C = c["C"]
    buf = torch.full((c["N"],) + c["hout"] + (C + 32,), 7.0, dtype=DT[c["dt"]], device="cuda")
    out = buf[..., 16:16 + C]                                                               # the middle slice
    K.edge_aspp(dev(inp["acts"]), dev(inp["w"]), dev(inp["scale"]), dev(inp["shift"]), out)
    reached(SEL, c)
    untouched(out, buf, off=16)
    assert_close(host(out), ref["y"], c["dt"], c["id"])


def test_edge_aspp_with_unit_weights_is_the_upsample_kernels_result(K):
    """w = scale = 1, shift = 0: every channel is relu of the C = 1 align-corners upsample of the same map."""
    acts = torch.rand(2, 5, 7, generator=torch.Generator().manual_seed(5)).cuda()
    out = torch.empty(2, 9, 13, 8, device="cuda")
    K.edge_aspp(acts, torch.ones(8, device="cuda"), torch.ones(8, device="cuda"), torch.zeros(8, device="cuda"), out)
    up = torch.relu(K.upsample_bilinear_ac(acts.unsqueeze(3).contiguous(), (9, 13)))
    assert torch.equal(out, up.expand(2, 9, 13, 8))


# ----------------------------------------------------------------------------------------------------------------- kd_rank1_add
R1 = S.cases_of("rank1_add")


@pytest.mark.parametrize("c", R1, ids=S.ids(R1))
def test_rank1_add(K, SEL, c):
    inp, ref = S.build(c)
    y, buf = view(inp["y0"], c["dt"], c["sliced"])
    K.rank1_add(y, dev(inp["g"]).reshape(-1), dev(inp["w"]), accumulate=c["acc"])
    reached(SEL, c)
    untouched(y, buf)
    assert_close(host(y), ref["y"], c["dt"], c["id"])


def test_rank1_add_refuses_channel_counts_that_are_no_multiple_of_8(K, SEL):
    from kdcc_amd import _lib
    C = S.R1_REFUSED_C
    y = torch.full(S.R1_SHAPE + (C,), 7.0, device="cuda")
    assert call(SEL, "rank1_add", 0, y.data_ptr(), C, 0x10000, C, y.numel() // C)["name"] == REFUSED
    marker = other_family_marker(K)
    with pytest.raises(_lib.KdccError):
        K.rank1_add(y, torch.zeros(S.R1_SHAPE, device="cuda").reshape(-1), torch.zeros(C, device="cuda"))
    assert _lib.last_plumbing_kernel() == marker and bool((y == 7.0).all()), "a refused call launched something"


# ---------------------------------------------------------------------------------------------------------------- kd_gated_conv
GC = S.cases_of("gated_conv")


@pytest.mark.parametrize("c", GC, ids=S.ids(GC))
def test_gated_conv(K, SEL, c):
    inp, ref = S.build(c)
    got, counts = run_gated_conv(K, c, inp)
    reached(SEL, c)
    assert counts == {c["kernel"]: 1}, f"{c['id']}: the launch went to {counts}, this row is meant to cover {c['kernel']}"
    assert_close(got, ref["y"], c["dt"], c["id"])


def test_gated_conv_bf16_valu_kernel_in_a_child_process():
    """gated_conv_kernel<bf16_t, C> runs only with KDCC_GATED_MFMA=0, which the library reads once per process: a fresh python
    runs C = 8 / 16 / 32 at 546 pixels against the float64 reference under the bf16 bars and asserts the kernel log."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KDCC_GATED_MFMA="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_shape_stream_child.py")], env=env, capture_output=True, text=True,
                       timeout=120, cwd=root)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert [l.split()[1] for l in r.stdout.splitlines() if l.startswith("ok ")] == S.ids(S.GC_VALU_BF16), r.stdout[-2000:]


# ----------------------------------------------------------------------------------------------------------- kd_pointwise_small
PW = S.cases_of("pointwise_small")


@pytest.mark.parametrize("c", PW, ids=S.ids(PW))
def test_pointwise_small(K, SEL, c):
    inp, ref = S.build(c)
    ci, co = c["cin"], c["cout"]
    shape = S.PW_NPIX[c["npix"]]
    xb = torch.full(shape + (ci + 16,), 7.0, dtype=torch.bfloat16, device="cuda")           # input: the first Cin channels
    xb[..., :ci] = dev(inp["x"], "bf16")
    ob = torch.full(shape + (co + S.PW_OUT_PAD,), 7.0, dtype=torch.bfloat16, device="cuda")
    out = ob[..., S.PW_OUT_OFF:S.PW_OUT_OFF + co]
    K.pointwise_small(xb[..., :ci], dev(inp["w"]), dev(inp["bias"]) if c["bias"] else None, out=out)
    reached(SEL, c)
    untouched(out, ob, off=S.PW_OUT_OFF)
    assert_close(host(out), ref["y"], "bf16", c["id"])


# ------------------------------------------------------------------------------------------------------------------------ kd_canny
CN = S.cases_of("canny")


@pytest.mark.parametrize("c", CN, ids=S.ids(CN))
def test_canny_reaches_the_hysteresis_fixed_point(K, SEL, c):
    """ops.canny with its default sweeps / max_rounds == oracle.canny_ref bit for bit: the line fixtures hang on one strong seed at
    the far end of a 1398-pixel weak chain, which takes canny_ref 1398 Jacobi rounds (more than the 8 x 64 sweeps ops.canny used to
    stop at, test_shape_stream_host.py)."""
    inp, ref = S.build(c)
    t0 = time.perf_counter()
    got, rounds = K.canny(dev(inp["x"]), S.CANNY_LOW, S.CANNY_HIGH, return_rounds=True)
    N, H, W = got.shape
    first, later = select(SEL, c), call(SEL, "canny_continue", N, H, W, 8)
    assert (first["name"], later["name"]) == (c["kernel"], c["then"])
    reached(SEL, c, first if rounds == 1 else later)          # kd_canny, then kd_canny_continue once per further round
    got = got.cpu().numpy()
    print(f"{c['id']}: {rounds} rounds of 8 sweeps on the device ({time.perf_counter() - t0:.3f} s), {ref['rounds']} Jacobi rounds in canny_ref")
    assert set(np.unique(got)) <= {0.0, 255.0}
    assert np.array_equal(got.astype(np.uint8), ref["edges"]), f"{c['id']}: {(got != ref['edges']).sum()} pixels differ after {rounds} rounds"
    assert torch.equal(K.canny(dev(inp["x"]), S.CANNY_LOW, S.CANNY_HIGH), torch.from_numpy(got).cuda())     # the plain return value


def test_canny_raises_when_max_rounds_is_reached_without_convergence(K):
    """A bound that binds raises (naming the size and the sweeps spent) instead of returning a partial map; one sweep per round:
    the chain cannot have grown 1398 pixels in 3 sweeps however the lanes race."""
    from kdcc_amd._lib import KdccError
    inp, ref = S.build(CN[0])
    with pytest.raises(KdccError, match=r"1 x 9 x 1400.*3 rounds \(3 sweeps\)"):
        K.canny(dev(inp["x"]), S.CANNY_LOW, S.CANNY_HIGH, sweeps=1, max_rounds=3)
