"""Case table of tests/test_shape_stream_gpu.py: one row per branch of the Gated-SCNN shape-stream kernels (csrc/gscnn_ops.hip,
csrc/gscnn_bwd.hip), the seeded inputs of each row and its float64 reference on the CPU, written from the module expressions
(models/gscnn.py; the reference's gate_spatial_conv.py:50-60 and gscnn.py:308-314).  No reference calls the library; nothing
here touches the device.  tests/test_shape_stream_host.py checks, without a GPU, that every reference runs and has the declared
shape, that the rows reach the branches they claim (the dispatch rules are restated below, their constants taken from
csrc/gscnn_select.h compiled for the host), and that the Canny fixtures need more hysteresis rounds than the old 8 x 64 sweep
budget.  Every row names the kernel its call notes (`kernel`, for the gated conv `slot`: slot_name); tests/test_gscnn_select_host.py
holds those names and the restated rules against the compiled selectors.

`build(case)` returns (inputs, reference): inputs are float32 numpy carriers already rounded to the storage dtype the row
gives that operand, references are float64.  Pixels are flattened: activations are (npix, C) unless a row says otherwise.
"""
import zlib

import numpy as np
import torch

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def q(a, dt):
    """Round to the kernel's storage dtype (round-to-nearest-even), back in a float32 carrier."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[dt]).float().numpy()


def rng_of(case):
    return np.random.default_rng(zlib.crc32(case["id"].encode()))


def sig(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def f64(a):
    return np.asarray(a, np.float64)


CASES = []


def case(op, cid, **kw):
    """A row.  `kernel` is the name the row's call leaves in the library's plumbing slot (csrc/gscnn_select.h's table; the
    gated-conv rows keep the conv log's name there and carry the slot's in `slot`, see slot_name)."""
    c = dict(op=op, id=f"{op}:{cid}", **kw)
    CASES.append(c)
    return c


def cases_of(*ops):
    return [c for c in CASES if c["op"] in ops]


def ids(cs):
    return [c["id"] for c in cs]


# ============================================================================================================ kd_small_linear
SL_TEMPLATES = (8, 16, 24, 40, 72)        # small_linear_kernel<COP>; tests/test_shape_stream_host.py holds them to the compiled header
SL_MAXC = 72


def sl_template(cout, templates=SL_TEMPLATES):
    """kd_small_linear's choice: the first instantiation that holds Cout."""
    return next(t for t in templates if cout <= t)


SL_PIX = 2 * 5 * 7
def _sl(cid, template, **kw):
    return case("small_linear", cid, kernel=f"small_linear_kernel<{template}>", **kw)


# both sides of every template boundary: (Cout, the template the row is written for)
for _co, _t in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 24), (24, 24), (25, 40), (40, 40), (41, 72), (72, 72)):
    for _ci in (1, 33, 72):
        _sl(f"co{_co}-ci{_ci}", _t, cin=_ci, cout=_co, x_dt="f32", x_slice=False, bias=False, relu=False, acc=None,
             mask=False)
for _co, _t in ((7, 8), (13, 16), (19, 24), (33, 40), (57, 72)):     # one row of each template for every operand form
    _sl(f"co{_co}-bf16-x-slice", _t, cin=33, cout=_co, x_dt="bf16", x_slice=True, bias=False, relu=False, acc=None, mask=False)
    _sl(f"co{_co}-bias-relu", _t, cin=33, cout=_co, x_dt="f32", x_slice=False, bias=True, relu=True, acc=None, mask=False)
    _sl(f"co{_co}-acc-f32-slice", _t, cin=33, cout=_co, x_dt="f32", x_slice=False, bias=True, relu=False, acc="f32", mask=False)
    _sl(f"co{_co}-acc-bf16-slice", _t, cin=33, cout=_co, x_dt="bf16", x_slice=True, bias=False, relu=False, acc="bf16", mask=False)
    _sl(f"co{_co}-mask-slice", _t, cin=33, cout=_co, x_dt="f32", x_slice=False, bias=False, relu=False, acc="f32", mask=True)
SL_REFUSED = [(73, 8), (8, 73)]                         # (Cin, Cout): one channel past SL_MAXC on either side


def build_small_linear(c):
    r = rng_of(c)
    ci, co = c["cin"], c["cout"]
    x = q(r.standard_normal((SL_PIX, ci)), c["x_dt"])
    w = (r.standard_normal((co, ci)) / np.sqrt(ci)).astype(np.float32)
    inp = {"x": x, "w": w}
    y = f64(x) @ f64(w).T
    if c["bias"]:
        inp["bias"] = (r.standard_normal(co) * 0.3).astype(np.float32)
        y = y + inp["bias"]
    if c["relu"]:
        y = np.maximum(y, 0)
    if c["mask"]:                                       # the backward through a ReLU whose output is `mask`
        inp["mask"] = np.maximum(r.standard_normal((SL_PIX, co)), 0).astype(np.float32)
        y = np.where(inp["mask"] > 0, y, 0.0)
    if c["acc"]:
        inp["y0"] = q(r.standard_normal((SL_PIX, co)), c["acc"])
        y = y + inp["y0"]
    return inp, {"y": y}


# ============================================================================================================= kd_small_wgrad
SW_CH, SW_PIX_PER_BLOCK, SW_MAX_BLOCKS, SW_THREADS = 64, 4096, 1024, 256


def sw_blocks(npix, per_block=SW_PIX_PER_BLOCK, max_blocks=SW_MAX_BLOCKS, chunk=SW_CH):
    """small_wgrad_blocks (gscnn_bwd.hip) -> (blocks, pixels per block)."""
    nb = min(max((npix + per_block - 1) // per_block, 1), max_blocks)
    pb = (npix + nb - 1) // nb
    pb = (pb + chunk - 1) // chunk * chunk
    return (npix + pb - 1) // pb, pb


def sw_workspace(ca, cb, npix, **kw):
    """kd_small_wgrad_workspace: one (Cb*Ca + Cb) fp32 partial per block."""
    return sw_blocks(npix, **kw)[0] * (ca * cb + cb) * 4


SW_PAIRS = [(24, 9), (8, 1), (2, 1), (33, 33), (17, 17), (72, 72), (72, 1), (1, 72)]     # (Ca, Cb)
SW_NPIX = [1, 63, 64, 65, 1479, 4096, 4097, 8300]
# the block rule in the regime no data row can reach (the 1024-block cap; there the round-up of the block's pixel count to whole
# 64-pixel chunks changes the number of blocks): checked through kd_small_wgrad_workspace, which allocates nothing
SW_PLAN_ONLY_NPIX = [4096 * 1024, 4096 * 1024 + 1024, 4096 * 1024 * 3 + 77]


def _sw(cid, ca, cb, npix, a_dt="f32", b_dt="f32", sliced=False, bias=True, acc=False, twice=False):
    return case("small_wgrad", cid, kernel="small_wgrad_partial_kernel", ca=ca, cb=cb, npix=npix, a_dt=a_dt, b_dt=b_dt, sliced=sliced, bias=bias, acc=acc, twice=twice)


for _ca, _cb in SW_PAIRS:                                # every channel pair at one block with a partial chunk and at two blocks
    for _n in (1479, 4097):
        _sw(f"{_ca}x{_cb}-n{_n}", _ca, _cb, _n)
for _n in SW_NPIX:                                       # every pixel count at the engine's 33 x 33, both storage types
    if _n not in (1479, 4097):
        _sw(f"33x33-n{_n}", 33, 33, _n)
    _sw(f"33x33-n{_n}-bf16", 33, 33, _n, a_dt="bf16", b_dt="bf16")
_sw("33x33-n4097-f32-bf16", 33, 33, 4097, a_dt="f32", b_dt="bf16")
_sw("33x33-n4097-bf16-f32", 33, 33, 4097, a_dt="bf16", b_dt="f32")
_sw("24x9-n1479-bf16-f32", 24, 9, 1479, a_dt="bf16", b_dt="f32")
_sw("72x72-n1479-bf16", 72, 72, 1479, a_dt="bf16", b_dt="bf16")
_sw("33x33-n4097-slices", 33, 33, 4097, sliced=True)
_sw("72x72-n1479-slices-bf16", 72, 72, 1479, a_dt="bf16", b_dt="bf16", sliced=True)
_sw("17x17-n4097-nobias", 17, 17, 4097, bias=False)
_sw("72x1-n1479-nobias", 72, 1, 1479, bias=False)
_sw("33x33-n4097-acc", 33, 33, 4097, acc=True)
_sw("72x72-n4097-acc-nobias", 72, 72, 4097, acc=True, bias=False)
_sw("17x17-n65-acc-bf16", 17, 17, 65, a_dt="bf16", b_dt="bf16", acc=True)
_sw("72x72-n4097-twice", 72, 72, 4097, a_dt="bf16", b_dt="f32", twice=True)        # the same call twice: bit-equal (fixed order)


def build_small_wgrad(c):
    r = rng_of(c)
    a = q(r.standard_normal((c["npix"], c["ca"])), c["a_dt"])
    b = q(r.standard_normal((c["npix"], c["cb"])), c["b_dt"])
    inp = {"a": a, "b": b}
    dw, db = f64(b).T @ f64(a), f64(b).sum(0)
    if c["acc"]:
        # of the size of the sums themselves (sqrt(npix)): a dropped or doubled accumulator shows
        s = np.sqrt(c["npix"])
        inp["dw0"], inp["db0"] = (r.standard_normal(dw.shape) * s).astype(np.float32), (r.standard_normal(db.shape) * s).astype(np.float32)
        dw, db = dw + inp["dw0"], db + inp["db0"]
    ref = {"dw": dw}
    if c["bias"]:
        ref["db"] = db
    return inp, ref


# ============================================================================================================ kd_gate_mix_bwd
GM_OUTS = ("all", "v-only", "grads-only")               # the three combinations engine.py asks for
for _C in (8, 16, 32):
    for _dt in ("f32", "bf16"):
        for _outs in GM_OUTS:
            for _shape in ((2, 6, 5), (1, 1, 1)):
                case("gate_mix_bwd", f"C{_C}-{_dt}-{_outs}-{'x'.join(map(str, _shape))}", C=_C, dt=_dt, outs=_outs, shape=_shape, kernel="gate_mix_bwd_kernel")


def build_gate_mix_bwd(c):
    r = rng_of(c)
    s, C = c["shape"], c["C"]
    feat = q(r.standard_normal(s + (C,)), c["dt"])
    a = r.standard_normal(s).astype(np.float32)
    inp, ref = {"feat": feat, "a": a}, {}
    al = sig(a)[..., None]
    if c["outs"] != "grads-only":
        ref["v"] = f64(feat) * (al + 1)
    if c["outs"] != "v-only":
        inp["gv"] = r.standard_normal(s + (C,)).astype(np.float32)
        ref["gfeat"] = f64(inp["gv"]) * (al + 1)
        ref["ga"] = (f64(inp["gv"]) * f64(feat)).sum(-1) * (al * (1 - al))[..., 0]
    return inp, ref


# ======================================================================================= kd_edge_attention (+ its backward)
for _op in ("edge_attention", "edge_attention_bwd"):
    for _dt in ("f32", "bf16"):
        for _n in (1, 255, 256, 257):                   # one thread, a ragged block, a full block, a second block
            case(_op, f"{_dt}-n{_n}", dt=_dt, npix=_n, kernel=f"edge_attention_kernel<{_dt}>" if _op == "edge_attention" else "edge_attention_bwd_kernel")


def _edge_operands(c, r):
    n = c["npix"]
    cs = q(r.standard_normal((1, 1, n, 8)), c["dt"])
    canny = ((r.random((1, 1, n)) < 0.3) * 255.0).astype(np.float32)
    w = (r.standard_normal(10) * 0.6).astype(np.float32)
    w[9] *= 0.02                                        # cw's weight on the 0 / 255 map: keeps the outer sigmoid off its rails
    eo = sig(f64(cs) @ f64(w[:8]))
    acts = sig(w[8] * eo + f64(w[9]) * canny)
    return {"cs": cs, "canny": canny, "w": w}, eo, acts


def build_edge_attention(c):
    inp, eo, acts = _edge_operands(c, rng_of(c))
    return inp, {"acts": acts}


def build_edge_attention_bwd(c):
    r = rng_of(c)
    inp, eo, acts = _edge_operands(c, r)
    inp["g"] = r.standard_normal(acts.shape).astype(np.float32)
    g_t = inp["g"] * acts * (1 - acts)
    return inp, {"g_t": g_t, "g_s": g_t * f64(inp["w"][8]) * eo * (1 - eo), "eo": eo, "canny": f64(inp["canny"])}


# =============================================================================================================== kd_edge_aspp
EA_SIZES = [((10, 14), (4, 6)),      # shrinking (the ratio the old test had)
            ((5, 7), (5, 7)),        # identity
            ((3, 4), (9, 13)),       # enlarging
            ((6, 9), (1, 1)),        # Ho == Wo == 1: the scale is 0
            ((1, 8), (3, 8)),        # H == 1: h1 clamps to h0
            ((7, 1), (7, 5))]        # W == 1
for (_hin, _hout) in EA_SIZES:
    for _C in (8, 16):
        for _dt in ("f32", "bf16"):
            case("edge_aspp", f"{_hin[0]}x{_hin[1]}to{_hout[0]}x{_hout[1]}-C{_C}-{_dt}", hin=_hin, hout=_hout, C=_C, dt=_dt, N=2, kernel=f"edge_aspp_kernel<{_dt}>")


def build_edge_aspp(c):
    from oracle import oracle as orc
    r = rng_of(c)
    C = c["C"]
    acts = r.random((c["N"],) + c["hin"]).astype(np.float32)
    w = r.standard_normal(C).astype(np.float32)
    sc = (r.random(C) + 0.5).astype(np.float32)
    sh = (r.standard_normal(C) * 0.1).astype(np.float32)
    e = f64(orc.upsample_bilinear_ac(acts[:, None], c["hout"])[:, 0])
    return {"acts": acts, "w": w, "scale": sc, "shift": sh}, {"y": np.maximum(e[..., None] * f64(w) * f64(sc) + f64(sh), 0)}


# =============================================================================================================== kd_rank1_add
for _C in (8, 32, 64):
    for _dt in ("f32", "bf16"):
        for _acc in (True, False):
            for _sl in (False, True):
                case("rank1_add", f"C{_C}-{_dt}-acc{int(_acc)}-{'slice' if _sl else 'dense'}", C=_C, dt=_dt, acc=_acc, sliced=_sl, kernel=f"rank1_add_kernel<{_dt}>")
R1_SHAPE = (2, 4, 6)
R1_REFUSED_C = 12


def build_rank1_add(c):
    r = rng_of(c)
    C = c["C"]
    y0 = q(r.standard_normal(R1_SHAPE + (C,)), c["dt"])     # accumulate = False must overwrite it
    g = r.standard_normal(R1_SHAPE).astype(np.float32)
    w = r.standard_normal(C).astype(np.float32)
    y = f64(g)[..., None] * f64(w)
    return {"y0": y0, "g": g, "w": w}, {"y": y + y0 if c["acc"] else y}


# ============================================================================================================== kd_gated_conv
GC_NPIX = {1: (1, 1, 1), 3: (1, 1, 3), 16: (1, 2, 8), 17: (1, 1, 17), 546: (2, 13, 21)}
for _C in (8, 16, 32):
    for _n in GC_NPIX:      # fewer pixels than a thread's group (4, or 2 at C = 32); one 16-pixel MFMA group, ragged ones
        case("gated_conv", f"C{_C}-n{_n}-f32", C=_C, npix=_n, dt="f32", kernel="gated_conv_kernel", slot=f"gated_conv_kernel<f32,{_C}>", round_w=False)
        case("gated_conv", f"C{_C}-n{_n}-bf16", C=_C, npix=_n, dt="bf16", kernel="gated_conv_mfma_kernel", slot=f"gated_conv_mfma_kernel<{_C}>", round_w=True)
# the bf16 VALU kernel (KDCC_GATED_MFMA=0, read once per process): run by a child process against the bf16 rows' reference
GC_VALU_BF16 = [c for c in CASES if c["op"] == "gated_conv" and c["dt"] == "bf16" and c["npix"] == 546]


def slot_name(c, mfma=True):
    """The name the row's call leaves in the plumbing slot; mfma=False: in the child process that runs GC_VALU_BF16."""
    if c["op"] == "gated_conv" and c["dt"] == "bf16" and not mfma:
        return f"gated_conv_kernel<bf16,{c['C']}>"
    return c.get("slot", c["kernel"])


def gate_params(c):
    """The packed fp32 vector kd_gated_conv documents: W1 (C+1, C+1), b1 (C+1), w2 (C+1), b2 (1), Wg (C, C)."""
    r = np.random.default_rng(zlib.crc32(f"gate-params-C{c['C']}".encode()))
    C, H = c["C"], c["C"] + 1
    return dict(W1=(r.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32), b1=(r.standard_normal(H) * 0.3).astype(np.float32),
                w2=(r.standard_normal(H) * 0.7).astype(np.float32), b2=(r.standard_normal(1) * 0.3).astype(np.float32),
                Wg=(r.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32))


def build_gated_conv(c):
    r = rng_of(c)
    C, shape = c["C"], GC_NPIX[c["npix"]]
    feat = q(r.standard_normal(shape + (C,)), c["dt"])
    gate = q(r.standard_normal(shape + (1,)), c["dt"])
    p = gate_params(c)
    prm = np.concatenate([p[k].reshape(-1) for k in ("W1", "b1", "w2", "b2", "Wg")]).astype(np.float32)
    W1, Wg = p["W1"].copy(), p["Wg"]
    if c["round_w"]:        # the matrix cores multiply bf16 W1[:, :C] and Wg; the gate column, b1, w2 and b2 stay fp32
        W1[:, :C] = q(W1[:, :C], "bf16")
        Wg = q(Wg, "bf16")
    u = np.concatenate([f64(feat), f64(gate)], -1)
    z = np.maximum(u @ f64(W1).T + f64(p["b1"]), 0)
    alpha = sig(z @ f64(p["w2"]) + f64(p["b2"][0]))
    y = (f64(feat) * (alpha[..., None] + 1)) @ f64(Wg).T
    return {"feat": feat, "gate": gate, "params": prm}, {"y": y}


# ========================================================================================================= kd_pointwise_small
PW_NPIX = {1: (1, 1, 1), 15: (1, 3, 5), 16: (1, 2, 8), 17: (1, 1, 17)}
for _ci, _co in ((64, 32), (32, 16), (16, 8)):
    for _n in PW_NPIX:
        case("pointwise_small", f"{_ci}to{_co}-n{_n}", cin=_ci, cout=_co, npix=_n, bias=True, kernel=f"pointwise_small_kernel<{_ci},{_co}>")
    case("pointwise_small", f"{_ci}to{_co}-n17-nobias", cin=_ci, cout=_co, npix=17, bias=False, kernel=f"pointwise_small_kernel<{_ci},{_co}>")
PW_OUT_PAD, PW_OUT_OFF = 12, 4      # the output: a slice at element 4 of a (Cout + 12)-wide buffer: ldy % 4 == 0, ldy % 8 != 0


def build_pointwise_small(c):
    r = rng_of(c)
    ci, co = c["cin"], c["cout"]
    x = q(r.standard_normal(PW_NPIX[c["npix"]] + (ci,)), "bf16")
    w = (r.standard_normal((co, ci)) / np.sqrt(ci)).astype(np.float32)
    inp = {"x": x, "w": w}
    y = f64(x) @ f64(q(w, "bf16")).T                   # the kernel rounds the weight to bf16 for the matrix cores
    if c["bias"]:
        inp["bias"] = r.standard_normal(co).astype(np.float32)
        y = y + inp["bias"]
    return inp, {"y": y}


# =================================================================================================================== kd_canny
CANNY_OLD_BUDGET = 8 * 64           # sweeps x max_rounds ops.canny used to stop at, converged or not
CANNY_LOW, CANNY_HIGH = 10, 100


def _canny_line(W=1400, H=9):
    """A step of 5 grey levels under row 4 (a weak edge along the whole row) that becomes a step of 40 (a strong edge) over the
    last 8 columns: the line is an edge only through hysteresis, from the one seed at its right end."""
    img = np.full((H, W), 100.0, np.float32)
    img[5:, :W - 8] += 5
    img[5:, W - 8:] += 40
    return img


# `kernel`: what kd_canny notes; `then`: what the kd_canny_continue rounds after it note (the line fixtures need them, the noise
# images may or may not)
case("canny", "line-seed-right", image="a", kernel="canny_grad_kernel", then="canny_hyst_kernel")            # grows against the index order, one neighbour per Jacobi round
case("canny", "line-seed-bottom", image="b", kernel="canny_grad_kernel", then="canny_hyst_kernel")           # the transpose: a vertical chain seeded at its lower end
case("canny", "line-seed-left", image="c", kernel="canny_grad_kernel", then="canny_hyst_kernel")             # the mirror image: grows with the index order
for _h, _w in ((1, 1), (1, 7), (2, 2), (3, 5)):        # border replication on images smaller than the 3x3 window; N = 2
    case("canny", f"noise-{_h}x{_w}", image="noise", hw=(_h, _w), kernel="canny_grad_kernel", then="canny_hyst_kernel")


def build_canny(c):
    """-> {"x": (N, 3, H, W) float32 batch}, {"edges": (N, H, W) uint8 0 / 255 from oracle.canny_ref, "rounds": its Jacobi rounds}."""
    from oracle import oracle as orc
    if c["image"] == "noise":
        h, w = c["hw"]
        x = rng_of(c).integers(0, 256, (2, 3, h, w)).astype(np.float32)
    else:
        a = _canny_line()
        g = {"a": a, "b": np.ascontiguousarray(a.T), "c": np.ascontiguousarray(a[:, ::-1])}[c["image"]]
        x = np.ascontiguousarray(np.broadcast_to(g, (1, 3) + g.shape))
    out = [orc.canny_ref(im.transpose(1, 2, 0).astype(np.uint8), CANNY_LOW, CANNY_HIGH, return_rounds=True) for im in x]
    return {"x": x}, {"edges": np.stack([o[0] for o in out]), "rounds": max(o[1] for o in out)}


# ============================================================================================================ kd_conv3x3_small
# Selection-only rows (not in CASES: no reference here): the calls tests/test_gscnn_gpu.py::test_conv3x3_small_vs_oracle makes, dense
# and as channel slices of 80-channel buffers, which is where the values are checked and the slot asserted.
C3_SHAPES = [(1, 16, 256), (2, 37, 45), (1, 20, 300), (1, 33, 513), (1, 3, 7)]
C3_LD = 80
C3_ROWS = [dict(op="conv3x3_small", id=f"conv3x3_small:C{_C}-{'x'.join(map(str, _s))}", C=_C, shape=_s, kernel=f"conv3x3_small_kernel<{_C}>")
           for _C in (16, 32, 64) for _s in C3_SHAPES]


BUILDERS = {"small_linear": build_small_linear, "small_wgrad": build_small_wgrad, "gate_mix_bwd": build_gate_mix_bwd,
            "edge_attention": build_edge_attention, "edge_attention_bwd": build_edge_attention_bwd, "edge_aspp": build_edge_aspp,
            "rank1_add": build_rank1_add, "gated_conv": build_gated_conv, "pointwise_small": build_pointwise_small, "canny": build_canny}


def build(c):
    return BUILDERS[c["op"]](c)


def expected_shapes(c):
    """{reference name: shape} each row declares, from its parameters alone."""
    op = c["op"]
    if op == "small_linear":
        return {"y": (SL_PIX, c["cout"])}
    if op == "small_wgrad":
        return {"dw": (c["cb"], c["ca"]), **({"db": (c["cb"],)} if c["bias"] else {})}
    if op == "gate_mix_bwd":
        s, out = c["shape"], {}
        if c["outs"] != "grads-only":
            out["v"] = s + (c["C"],)
        if c["outs"] != "v-only":
            out.update(gfeat=s + (c["C"],), ga=s)
        return out
    if op == "edge_attention":
        return {"acts": (1, 1, c["npix"])}
    if op == "edge_attention_bwd":
        s = (1, 1, c["npix"])
        return {"g_t": s, "g_s": s, "eo": s, "canny": s}
    if op == "edge_aspp":
        return {"y": (c["N"],) + c["hout"] + (c["C"],)}
    if op == "rank1_add":
        return {"y": R1_SHAPE + (c["C"],)}
    if op == "gated_conv":
        return {"y": GC_NPIX[c["npix"]] + (c["C"],)}
    if op == "pointwise_small":
        return {"y": PW_NPIX[c["npix"]] + (c["cout"],)}
    if op == "canny":
        if c["image"] == "noise":
            return {"edges": (2,) + c["hw"]}
        return {"edges": (1, 1400, 9) if c["image"] == "b" else (1, 9, 1400)}
    raise KeyError(op)
