"""Case table of tests/test_loss_dispatch_gpu.py: one row per dispatch branch of the criterion, metric and optimizer entry
points of csrc/losses.hip, rows on both sides of every numeric gate, a grid-stride second trip per capped grid, tails, views of
wider buffers and values that bite; the seeded inputs of each row and its float64 reference on the CPU.

Every row names the kernel it is meant to reach (`kernel`: the name the launcher notes, loss_kernel_name() of csrc/loss_select.h)
and `rule(c)` predicts that name from the row alone, by a restatement of the family's selector in csrc/loss_select.h (the source
lines are quoted next to each restatement).  tests/test_loss_dispatch_host.py checks, without a GPU, that every name of the table has
a row, that every row's rule gives the row's name and that every reference runs; tests/test_loss_select_host.py holds the compiled
selectors against the rules.  Nothing here touches the device or the library.

Operands are logical (N, C, H, W) or (N, C) arrays; a row's `lay` says how each one lies in memory:
  "nchw"  dense, pixels fastest        "cl"      dense channels-last (the engine's logits layout)
  "cs"    a channel slice of a channels-last buffer of C + 16 channels, at channel 8
  "bs"    a batch slice: channels-last images with one spare pixel row each (sN != C * P)
  "off1"  dense channels-last, the base one fp32 / bf16 element past a 16-B boundary
  "2d"    (N, C) rows                  "2ds"     (N, C) rows of a (N, C + 16) buffer, at column 8
`build(case)` returns (inputs, reference): inputs already rounded to the storage dtype (float32 carriers), references float64.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import _criteria_ref as CR
import _ensemble_ref as ER

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
U = 2.0 ** -24
MAX_BLOCKS = 2048                       # loss_select.h: "constexpr int LOSS_MAX_BLOCKS = 2048;"
FOCAL_MAX_BLOCKS = 2 * MAX_BLOCKS // 3  # "constexpr int LOSS_FOCAL_MAX_BLOCKS = 2 * LOSS_MAX_BLOCKS / 3;"
MT_MAX_BLOCKS = 2 * MAX_BLOCKS // 3     # "constexpr int LOSS_MT_MAX_BLOCKS = 2 * LOSS_MAX_BLOCKS / 3;"
MET_MAX_BLOCKS = MAX_BLOCKS // 2        # "constexpr int LOSS_MET_MAX_BLOCKS = LOSS_MAX_BLOCKS / 2;"
UP_NW = 160                             # "constexpr int LOSS_UP_NW = 160;"
LDS = 65536                             # "constexpr size_t LOSS_LDS_DEFAULT = 65536;": the default dynamic-LDS limit the gates compare with
RADAM_BLK = 256 * 8                     # losses.hip: "constexpr int RADAM_BLK = 256 * 8;"
KD_MULTI_MAX = 16                       # include/kdcc.h
SENTINEL = 7.0


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the bound on a chain of n fp32 roundings."""
    return n * U / (1.0 - n * U)


def q(a, dt):
    """Round to the storage dtype (round-to-nearest-even), back in a float32 carrier."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[dt]).float().numpy()


def rng_of(case, salt=0):
    return np.random.default_rng(zlib.crc32(case["id"].encode()) + salt)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


CASES = []


def case(op, cid, kernel, **kw):
    c = dict(op=op, id=f"{op}:{cid}", kernel=kernel, **kw)
    CASES.append(c)
    return c


def cases_of(*ops):
    return [c for c in CASES if c["op"] in ops]


def ids(cs):
    return [c["id"] for c in cs]


# =================================================================================================== layouts and their strides
def dims(c):
    """(N, C, P) as ops.view3 reports them."""
    s = c["shape"]
    return (s[0], s[1], 1) if len(s) == 2 else (s[0], s[1], s[2] * s[3])


def strides(lay, shape):
    """Element strides (sN, sC, sP) of a logical operand, as ops.view3 hands them to the library."""
    if len(shape) == 2:
        N, C = shape
        return {"2d": (C, 1, 0), "2ds": (C + 16, 1, 0)}[lay]
    N, C, H, W = shape
    P = H * W
    return {"nchw": (C * P, P, 1), "cl": (C * P, 1, C), "off1": (C * P, 1, C), "cs": (P * (C + 16), 1, C + 16),
            "bs": (C * (P + W), 1, C)}[lay]


def aligned16(lay, dt):
    """Is the operand's base 16-B aligned?  Buffers are (allocator: 256-B aligned); a slice starts 8 elements in."""
    esz = 2 if dt == "bf16" else 4
    return {"nchw": True, "cl": True, "bs": True, "2d": True, "off1": False, "cs": (8 * esz) % 16 == 0, "2ds": (8 * esz) % 16 == 0}[lay]


def lays(c):
    """(s, t, grad) layouts of a two-operand row; grad None when the row asks for no gradient."""
    l = c["lay"]
    return (l, l, l if c.get("gdt", c["sdt"]) else None) if isinstance(l, str) else l


def blocks_for(total):
    """loss_select.h loss_blocks_for(), cap = LOSS_MAX_BLOCKS: "const long long b = (total + 255) / 256; return (int)(b < 1 ? 1 : (b > cap ? cap : b));" """
    return max(1, min((total + 255) // 256, MAX_BLOCKS))


def nhwc(st, N, C, P):
    """loss_select.h loss_nhwc(): "return v->sC == 1 && v->sP == C && (v->sN == (int64_t)C * P || N == 1);" (every family asks it)."""
    sN, sC, sP = st
    return sC == 1 and sP == C and (sN == C * P or N == 1)


def dense_same(c):
    """loss_select.h loss_dense_same(): every operand dense in one of the two orders ("(a->sC == 1 && a->sP == C && a->sN == C * P) ||
    (a->sP == 1 && a->sC == P && a->sN == C * P)"), "a->sN != b->sN || ... || a->dtype != b->dtype" -> false, the same for g,
    "!loss_aligned16(a->ptr) || !loss_aligned16(b->ptr) || (g && !loss_aligned16(g->ptr))" -> false, then
    "return ((long long)N * C * P) % 8 == 0;" """
    N, C, P = dims(c)
    ls, lt, lg = lays(c)
    sdt, tdt, gdt = c["sdt"], c["tdt"], c.get("gdt", c["sdt"])
    a = strides(ls, c["shape"])
    if not ((a[1] == 1 and a[2] == C and a[0] == C * P) or (a[2] == 1 and a[1] == P and a[0] == C * P)):
        return False
    if strides(lt, c["shape"]) != a or tdt != sdt:
        return False
    if lg is not None and (strides(lg, c["shape"]) != a or gdt != sdt):
        return False
    if not aligned16(ls, sdt) or not aligned16(lt, tdt) or (lg is not None and not aligned16(lg, gdt)):
        return False
    return (N * C * P) % 8 == 0


# ============================================================================== the two-operand criteria: kldiv / jsdiv / ensemble_kldiv
def pair_rule(c):
    """loss_select_pair: "const size_t lds = (size_t)2 * 256 * C * sizeof(float);"
    "if (lds <= LOSS_LDS_DEFAULT && loss_nhwc(s, N, C, P) && loss_nhwc(t, N, C, P) && (!grad || loss_nhwc(grad, N, C, P)))" then
    "LK_PAIR_NHWC + 8 * kind + 4 * (s->dtype == KD_BF16) + 2 * (t->dtype == KD_BF16) + (gdt == KD_BF16)" with
    "const int gdt = grad ? grad->dtype : s->dtype;", else "LK_PAIR_KLD + kind" """
    N, C, P = dims(c)
    fast = 2 * 256 * C * 4 <= LDS and all(nhwc(strides(l, c["shape"]), N, C, P) for l in lays(c) if l is not None)
    if not fast:
        return f"pair_kernel<{c['kind']}>"
    return f"pair_nhwc_kernel<{c['kind']},{c['sdt']},{c['tdt']},{c.get('gdt') or c['sdt']}>"


def _pair(kind, cid, shape, lay="cl", sdt="f32", tdt="f32", T=2.0, **kw):
    c = dict(op="pair", id=f"pair:{kind}-{cid}", kind=kind, shape=shape, lay=lay, sdt=sdt, tdt=tdt, T=T, **kw)
    c.setdefault("gdt", sdt)
    c["kernel"] = pair_rule(c) if "kernel" not in kw else kw["kernel"]
    CASES.append(c)
    return c


for _k in ("kld", "jsd", "ekl"):
    # the eight storage-type forms of the NHWC kernel (2 x 126 pixels: a ragged block); a gradient of the other type than the
    # student's is what the library's C interface allows and no Python wrapper asks for
    for _s in ("f32", "bf16"):
        for _t in ("f32", "bf16"):
            for _g in ("f32", "bf16"):
                _pair(_k, f"nhwc-{_s}-{_t}-{_g}", (2, 19, 9, 14), sdt=_s, tdt=_t, gdt=_g, kernel=f"pair_nhwc_kernel<{_k},{_s},{_t},{_g}>")
    _pair(_k, "nchw", (2, 19, 9, 14), lay="nchw", kernel=f"pair_kernel<{_k}>")
    _pair(_k, "nchw-bf16", (2, 19, 9, 14), lay="nchw", sdt="bf16", tdt="bf16", kernel=f"pair_kernel<{_k}>")
    _pair(_k, "2d", (37, 10), lay="2d", kernel=f"pair_kernel<{_k}>")                   # (N, C): sP = 0, never the NHWC test
    _pair(_k, "nograd", (2, 19, 9, 14), gdt=None, kernel=f"pair_nhwc_kernel<{_k},f32,f32,f32>")
    # the LDS gate: 2 x 256 x 32 x 4 B = 64 KiB exactly
    _pair(_k, "C32", (1, 32, 9, 31), kernel=f"pair_nhwc_kernel<{_k},f32,f32,f32>", gate=("pair-lds", _k, 0))
    _pair(_k, "C33", (1, 33, 9, 31), kernel=f"pair_kernel<{_k}>", gate=("pair-lds", _k, 1))
    # each operand in turn as a channel slice: the strided kernel; the buffer around a sliced gradient keeps its sentinel
    for _i, _nm in enumerate("stg"):
        _l = ["cl", "cl", "cl"]
        _l[_i] = "cs"
        _pair(_k, f"cslice-{_nm}", (2, 19, 5, 7), lay=tuple(_l), kernel=f"pair_kernel<{_k}>")
    _pair(_k, "cslice-all", (2, 19, 5, 7), lay="cs", kernel=f"pair_kernel<{_k}>")
    _pair(_k, "bslice", (2, 19, 5, 7), lay="bs", kernel=f"pair_kernel<{_k}>")
    _pair(_k, "bslice-N1", (1, 19, 5, 7), lay="bs", kernel=f"pair_nhwc_kernel<{_k},f32,f32,f32>")     # "|| N == 1"
    _pair(_k, "bslice-g-only", (2, 19, 5, 7), lay=("cl", "cl", "bs"), kernel=f"pair_kernel<{_k}>")
    # logits spread over +-30: the max subtraction matters.  Marked ill-conditioned, so the GPU test takes max(project bar, 3 x the
    # deviation of pair_formula evaluated in fp32 on the CPU) and prints both; measured, that deviation is 5e-7 (kld), 7e-6 (jsd)
    # and 1e-7 (ekl) in losses of 25 to 300 and 4e-7 / 7e-7 / 3e-7 of the gradient's range: the project bars decide after all
    _pair(_k, "spread30", (2, 19, 9, 14), spread=30.0, illcond=True, kernel=f"pair_nhwc_kernel<{_k},f32,f32,f32>")
    _pair(_k, "spread30-nchw", (2, 19, 9, 14), lay="nchw", spread=30.0, illcond=True, kernel=f"pair_kernel<{_k}>")
# 525 001 pixels of 3 classes: more than 2048 blocks of 256, a ragged last block
_pair("kld", "second-trip", (1, 3, 525, 1000 + 1), second_trip=(525 * 1001, MAX_BLOCKS), chain=("inside", "per-pixel KL values of order 0.1 over 5e5 pixels: partial sums stay near 2^16, one chain loses 1e-6 relative"))
_pair("jsd", "second-trip-nchw", (3, 3, 175, 1001), lay="nchw", second_trip=(3 * 175 * 1001, MAX_BLOCKS), chain=("inside", "as the KL row"))
_pair("ekl", "second-trip", (1, 3, 525, 1001), sdt="bf16", tdt="bf16", second_trip=(525 * 1001, MAX_BLOCKS), chain=("inside", "as the KL row"))
# one class 200 below the rest in both operands: ps + pt underflows there and jsd_log_q takes its log-space arm
_pair("jsd", "underflow", (2, 19, 9, 14), low200=True, T=1.0)
_pair("jsd", "underflow-nchw", (2, 19, 9, 14), lay="nchw", low200=True, T=1.0)
# a target row with exact zeros: xlogy(0, 0) = 0
_pair("ekl", "zeros", (2, 19, 9, 14), tzeros=True)
_pair("ekl", "zeros-nchw", (2, 19, 9, 14), lay="nchw", tzeros=True)


def pair_formula(kind, s, t, T):
    """(per-pixel values, loss scale, gradient) of losses/KLDiv.py, JSDiv.py, EnsembleKLDiv.py in the dtype of s and t; s, t are
    (N, C, ...) torch tensors.  loss = scale * sum(values)."""
    N, C = s.shape[:2]
    NP = s.numel() // C
    if kind == "ekl":
        lps = F.log_softmax(s, 1)
        return (torch.xlogy(t, t) - t * lps).sum(1), 1.0 / NP, (lps.exp() * t.sum(1, keepdim=True) - t) / NP
    lps, lpt = F.log_softmax(s / T, 1), F.log_softmax(t / T, 1)
    ps, pt = lps.exp(), lpt.exp()
    if kind == "kld":
        return (torch.xlogy(pt, pt) - pt * lps).sum(1), T * T / NP, T / NP * (ps - pt)
    lq = math.log(0.5) + torch.logaddexp(lps, lpt)
    a = lps - lq
    return (torch.xlogy(ps, ps) + torch.xlogy(pt, pt) - (ps + pt) * lq).sum(1), T * T / (2 * N), T / (2 * N) * ps * (a - (ps * a).sum(1, keepdim=True))


def build_pair(c):
    r = rng_of(c)
    shape, kind = c["shape"], c["kind"]
    sp = c.get("spread", 3.0)
    s = r.uniform(-sp, sp, shape) if "spread" in c else r.standard_normal(shape) * 2
    t = r.uniform(-sp, sp, shape) if "spread" in c else r.standard_normal(shape) * 2
    if c.get("low200"):
        s[:, 5] -= 200.0
        t[:, 5] -= 200.0
    if kind == "ekl":
        t = torch.softmax(t64(t), 1).numpy()
        if c.get("tzeros"):
            t[:, 3] = 0.0
            t[:, 11] = 0.0
    s, t = q(s, c["sdt"]), q(t, c["tdt"])
    vals, scale, grad = pair_formula(kind, t64(s), t64(t), c["T"])
    ref = {"loss": float(vals.sum() * scale), "terms": vals.numpy().ravel(), "scale": scale}
    if c.get("gdt"):
        ref["grad"] = grad.numpy()
    if c.get("illcond"):
        v32, _, g32 = pair_formula(kind, torch.from_numpy(s), torch.from_numpy(t), c["T"])
        ref["loss32"] = float(v32.double().sum() * scale)
        ref["grad32"] = g32.double().numpy()
    return {"s": s, "t": t}, ref


# ================================================================================================================ kd_hint_mse
def mse_rule(c):
    """loss_select_mse: "if (loss_dense_same(s, t, grad, N, C, P)) return loss_flat((LossKernel)(LK_MSE_VEC_F32 + (s->dtype == KD_BF16)),
    numel / 8);" else "return loss_flat(LK_MSE_STRIDED, numel);" """
    if dense_same(c):
        return f"mse_vec_kernel<{c['sdt']}>"
    return "mse_strided_kernel"


def _mse(cid, shape, lay="cl", dt="f32", **kw):
    c = dict(op="hint_mse", id=f"hint_mse:{cid}", shape=shape, lay=lay, sdt=dt, tdt=kw.pop("tdt", dt), **kw)
    c.setdefault("gdt", dt)
    c["kernel"] = kw.get("kernel") or mse_rule(c)
    CASES.append(c)
    return c


SHORT = "a few thousand terms at most: one fp32 chain is no longer than the bound allows"
for _dt in ("f32", "bf16"):
    _mse(f"vec-cl-{_dt}", (2, 24, 5, 7), dt=_dt, kernel=f"mse_vec_kernel<{_dt}>", gate=("mse-numel8", _dt, 0), chain=("inside", SHORT))
    _mse(f"vec-nchw-{_dt}", (2, 24, 5, 7), lay="nchw", dt=_dt, kernel=f"mse_vec_kernel<{_dt}>", chain=("inside", SHORT))
    _mse(f"numel-rem4-{_dt}", (1, 12, 5, 7), dt=_dt, kernel="mse_strided_kernel", gate=("mse-numel8", _dt, 1), chain=("inside", SHORT))   # 420 = 8 * 52 + 4
    _mse(f"aligned-{_dt}", (1, 8, 5, 7), dt=_dt, kernel=f"mse_vec_kernel<{_dt}>", gate=("mse-align", _dt, 0), chain=("inside", SHORT))
    _mse(f"off1-{_dt}", (1, 8, 5, 7), lay="off1", dt=_dt, kernel="mse_strided_kernel", gate=("mse-align", _dt, 1), chain=("inside", SHORT))
    _mse(f"cslice-g-{_dt}", (2, 24, 5, 7), lay=("cl", "cl", "cs"), dt=_dt, kernel="mse_strided_kernel", chain=("inside", SHORT))
    _mse(f"bslice-{_dt}", (2, 24, 5, 7), lay="bs", dt=_dt, kernel="mse_strided_kernel", chain=("inside", SHORT))
_mse("mixed-dtypes", (2, 24, 5, 7), dt="f32", tdt="bf16", kernel="mse_strided_kernel", chain=("inside", SHORT))
_mse("nograd", (2, 24, 5, 7), gdt=None, kernel="mse_vec_kernel<f32>", chain=("inside", SHORT))
# 4 204 032 elements: 525 504 octets > 2048 x 256 threads; (s - t)^2 of order 2: one fp32 chain loses 1e-4 relative
_mse("second-trip-vec-f32", (1, 8, 513, 1024), second_trip=(513 * 1024, MAX_BLOCKS), chain=("bites", ("loss",)))
_mse("second-trip-vec-bf16", (1, 8, 513, 1024), dt="bf16", second_trip=(513 * 1024, MAX_BLOCKS), chain=("bites", ("loss",)))
# 525 004 elements, one per thread, numel % 8 = 4
_mse("second-trip-strided", (1, 4, 131251, 1), lay="nchw", second_trip=(525004, MAX_BLOCKS), chain=("bites", ("loss",)))


def mse_chain(c):
    """The longest fp32 chain of the kernel's own decomposition.  mse_vec_kernel: "acc = fmaf(d[q], d[q], acc)" 8 times a step,
    "if (++cnt == 16) { dacc += (double)acc; acc = 0.f; cnt = 0; }": 128 roundings; mse_strided_kernel: "acc += (double)d * d": none.
    k = 3: the difference, the fp64 -> fp32 store, one to spare for the scale."""
    return (128 if c["kernel"].startswith("mse_vec") else 0) + 3


def build_mse(c):
    r = rng_of(c)
    s, t = q(r.standard_normal(c["shape"]), c["sdt"]), q(r.standard_normal(c["shape"]), c["tdt"])
    d = s.astype(np.float64) - t
    nc = c.get("num_classes", 19.0)
    ref = {"loss": float((d * d).sum() * nc / d.size), "terms": (d * d).ravel(), "scale": nc / d.size}
    if c["chain"][0] == "bites":      # (the other rows are held to the project's rtol = 1e-4)
        ref["bound"] = gamma(mse_chain(c)) * ref["loss"]
    if c.get("gdt"):
        ref["grad"] = 2.0 * nc / d.size * d
    return {"s": s, "t": t, "num_classes": nc}, ref


# ======================================================================================================= kd_weighted_hint_mse
def whmse_plan(P):
    """loss_select_whmse: "c.chunks = (int)(P < LOSS_WHMSE_MAX_CHUNKS ? P : LOSS_WHMSE_MAX_CHUNKS);" (64)
    "c.per_chunk = c.chunks > 0 ? (P + c.chunks - 1) / c.chunks : 0;"
    -> (chunks, per_chunk, empty trailing chunks, pixels of the last non-empty chunk)."""
    chunks = P if P < 64 else 64
    per = (P + chunks - 1) // chunks
    used = (P + per - 1) // per
    return chunks, per, chunks - used, P - (used - 1) * per


def _wh(cid, shape, lay="nchw", per_sample=False, dt="f32", **kw):
    kw.setdefault("gdt", dt)
    c = case("whmse", cid, "whmse_kernel", shape=shape, lay=lay, per_sample=per_sample, sdt=dt, tdt=dt, **kw)
    c["chain"] = ("inside", "a thread's chain is one channel's share of a chunk; the row checks indexing")
    return c


for _ps in (False, True):
    _tag = "per-sample" if _ps else "shared"
    _wh(f"P30-{_tag}", (2, 24, 5, 6), per_sample=_ps, plan=(30, 1, 0, 1))               # P < 64: one pixel a chunk
    _wh(f"P65-{_tag}", (2, 24, 5, 13), per_sample=_ps, plan=(64, 2, 31, 1))             # 31 empty trailing chunks, a ragged last one
    _wh(f"P100-{_tag}", (2, 24, 10, 10), per_sample=_ps, lay="cl", plan=(64, 2, 14, 2))  # 14 empty trailing chunks
    _wh(f"P4097-{_tag}", (2, 8, 17, 241), per_sample=_ps, plan=(64, 65, 0, 2))           # ragged last chunk (2 of 65)
_wh("C260-two-channel-blocks", (1, 260, 5, 13), per_sample=True, plan=(64, 2, 31, 1))
_wh("P100-bf16", (2, 24, 10, 10), dt="bf16", lay="cl", plan=(64, 2, 14, 2))
_wh("P65-cslice-g", (2, 24, 5, 13), lay=("cl", "cl", "cs"), per_sample=True, plan=(64, 2, 31, 1))
_wh("P65-nograd", (2, 24, 5, 13), gdt=None, plan=(64, 2, 31, 1))


def build_whmse(c):
    """losses/WeightedHintMSELoss.py:5-16: mean_n( sum_c w * mean_p (s - t)^2 / sum_c w )."""
    r = rng_of(c)
    N, C, P = dims(c)
    s, t = q(r.standard_normal(c["shape"]), c["sdt"]), q(r.standard_normal(c["shape"]), c["tdt"])
    w = (np.abs(r.standard_normal((N, C) if c["per_sample"] else (C,))) + 0.1).astype(np.float32)
    wn = w.astype(np.float64) if c["per_sample"] else np.broadcast_to(w.astype(np.float64), (N, C))
    d = (s.astype(np.float64) - t).reshape(N, C, P)
    per = (d * d).mean(2) * wn / wn.sum(1, keepdims=True)
    ref = {"loss": float(per.sum() / N), "terms": per.ravel(), "scale": 1.0 / N}
    if c.get("gdt"):
        ref["grad"] = (2.0 * d * (wn / wn.sum(1, keepdims=True))[:, :, None] / (N * P)).reshape(c["shape"])
    return {"s": s, "t": t, "w": w}, ref


# ======================================================================================= kd_ce2d / kd_ce2d_weighted and their gradient
def ce_rule(c):
    """loss_select_ce2d: "const size_t lds = (size_t)256 * C * sizeof(float);" "if (lds <= LOSS_LDS_DEFAULT && loss_nhwc(x, N, C, P))"
    -> ce2d_nhwc_kernel<float | bf16_t>, else ce2d_kernel"""
    N, C, P = dims(c)
    if 256 * C * 4 <= LDS and nhwc(strides(c["lay"], c["shape"]), N, C, P):
        return f"ce2d_nhwc_kernel<{c['dt']}>"
    return "ce2d_kernel"


def _ce(cid, shape, lay="cl", dt="f32", **kw):
    c = dict(op="ce2d", id=f"ce2d:{cid}", shape=shape, lay=lay, dt=dt, **kw)
    c["kernel"] = kw.get("kernel") or ce_rule(c)
    CASES.append(c)
    return c


for _dt in ("f32", "bf16"):
    _ce(f"nhwc-{_dt}", (2, 19, 9, 14), dt=_dt, kernel=f"ce2d_nhwc_kernel<{_dt}>")
    _ce(f"nchw-{_dt}", (2, 19, 9, 14), lay="nchw", dt=_dt, kernel="ce2d_kernel")
_ce("C64", (1, 64, 9, 31), kernel="ce2d_nhwc_kernel<f32>", gate=("ce-lds", 0))      # 256 x 64 x 4 B = 64 KiB exactly
_ce("C65", (1, 65, 9, 31), kernel="ce2d_kernel", gate=("ce-lds", 1))
_ce("cslice", (2, 19, 5, 7), lay="cs", kernel="ce2d_kernel")
_ce("bslice", (2, 19, 5, 7), lay="bs", kernel="ce2d_kernel")
_ce("bslice-N1", (1, 19, 5, 7), lay="bs", kernel="ce2d_nhwc_kernel<f32>")
_ce("2d", (37, 10), lay="2d", kernel="ce2d_kernel")
for _lay in ("cl", "nchw"):
    _ce(f"weighted-{_lay}", (2, 19, 9, 14), lay=_lay, weight=True)
    _ce(f"weighted-sum-{_lay}", (2, 19, 9, 14), lay=_lay, weight=True, size_average=False)
    _ce(f"sum-{_lay}", (2, 19, 9, 14), lay=_lay, size_average=False)
    _ce(f"spread30-{_lay}", (2, 19, 9, 14), lay=_lay, spread=30.0)
    _ce(f"all-ignored-{_lay}", (2, 19, 9, 14), lay=_lay, all_ignored=True)
    _ce(f"out-of-range-{_lay}", (2, 19, 9, 14), lay=_lay, out_of_range=True)
CE_INSIDE = "per-pixel losses of order 1 over 5e5 pixels: one chain's partial sums stay below 2^20"
_ce("second-trip-nhwc", (1, 3, 525, 1001), second_trip=(525 * 1001, MAX_BLOCKS), chain=("inside", CE_INSIDE))
_ce("second-trip-nchw", (3, 3, 175, 1001), lay="nchw", second_trip=(3 * 175 * 1001, MAX_BLOCKS), chain=("inside", CE_INSIDE))

for _lay in ("cl", "nchw", "cs", "bs"):
    case("ce2d_grad", f"plain-{_lay}", "ce2d_grad_kernel", shape=(2, 19, 5, 7), lay=_lay, dt="f32")
case("ce2d_grad", "bf16", "ce2d_grad_kernel", shape=(2, 19, 9, 14), lay="cl", dt="bf16")
case("ce2d_grad", "weighted", "ce2d_grad_kernel", shape=(2, 19, 9, 14), lay="cl", dt="f32", weight=True)
case("ce2d_grad", "weighted-sum", "ce2d_grad_kernel", shape=(2, 19, 9, 14), lay="nchw", dt="f32", weight=True, size_average=False)
case("ce2d_grad", "sum", "ce2d_grad_kernel", shape=(2, 19, 9, 14), lay="cl", dt="f32", size_average=False)
case("ce2d_grad", "spread30", "ce2d_grad_kernel", shape=(2, 19, 9, 14), lay="cl", dt="f32", spread=30.0)
case("ce2d_grad", "all-ignored", "ce2d_grad_kernel", shape=(2, 19, 9, 14), lay="cl", dt="f32", all_ignored=True)
case("ce2d_grad", "out-of-range", "ce2d_grad_kernel", shape=(2, 19, 9, 14), lay="nchw", dt="f32", out_of_range=True)
case("ce2d_grad", "second-trip", "ce2d_grad_kernel", shape=(1, 3, 525, 1001), lay="cl", dt="f32", second_trip=(525 * 1001, MAX_BLOCKS))


def labels_of(c, r, N, C, sp):
    """int64 labels: a tenth ignored (255 unless the row says otherwise), optionally all ignored or some outside [0, C)."""
    ign = c.get("ignore_index", 255)
    y = r.integers(0, C, size=(N,) + tuple(sp)).astype(np.int64)
    y[r.random(y.shape) < 0.1] = ign
    if c.get("all_ignored"):
        y[:] = ign
    if c.get("out_of_range"):
        m = r.random(y.shape)
        y[m < 0.1] = -3
        y[(m >= 0.1) & (m < 0.2)] = C + 5
    return y


def ce_formula(x, y, w, size_average, ignore_index):
    """losses/CrossEntropy.py:5-14 (nn.NLLLoss(weight, size_average, ignore_index) of log_softmax) -> (per-pixel weighted
    losses, weight sum, loss, gradient); labels outside [0, C) are skipped like the ignored ones (ce2d_kernel)."""
    N, C = x.shape[:2]
    lp = F.log_softmax(x, 1)
    valid = (y != ignore_index) & (y >= 0) & (y < C)
    yc = torch.where(valid, y, torch.zeros_like(y))
    wy = torch.where(valid, (torch.ones(C, dtype=x.dtype) if w is None else w)[yc], torch.zeros((), dtype=x.dtype))
    nll = -wy * lp.gather(1, yc.unsqueeze(1)).squeeze(1)
    tot = wy.sum()
    onehot = torch.zeros_like(x).scatter_(1, yc.unsqueeze(1), 1.0)
    g = wy.unsqueeze(1) * (lp.exp() - onehot)
    if size_average:
        loss = nll.sum() / tot if tot > 0 else torch.zeros((), dtype=x.dtype)
        g = g / tot if tot > 0 else torch.zeros_like(g)
    else:
        loss = nll.sum()
    return nll, tot, loss, g


def build_ce(c):
    r = rng_of(c)
    shape = c["shape"]
    N, C = shape[:2]
    x = q(r.uniform(-c["spread"], c["spread"], shape) if "spread" in c else r.standard_normal(shape) * 2, c["dt"])
    y = labels_of(c, r, N, C, shape[2:])
    w = (np.abs(r.standard_normal(C)) + 0.2).astype(np.float32) if c.get("weight") else None
    nll, tot, loss, g = ce_formula(t64(x), torch.from_numpy(y), None if w is None else t64(w), c.get("size_average", True), c.get("ignore_index", 255))
    ref = {"loss": float(loss), "grad": g.numpy(), "terms": nll.numpy().ravel(), "scale": 1.0 / max(float(tot), 1e-300) if c.get("size_average", True) else 1.0}
    return {"x": x, "y": y, "w": w}, ref


# ============================================================================================================== kd_confusion
def conf_rule(c):
    """loss_select_confusion: "hist = (size_t)C * C * sizeof(unsigned int), lds = (size_t)256 * C * sizeof(float) + hist;"
    "if (lds <= LOSS_LDS_DEFAULT && loss_nhwc(x, N, C, P))" -> confusion_nhwc_kernel<float | bf16_t>, else confusion_kernel.
    256 * 4 * C + 4 * C^2 <= 65536 holds up to C = 53 (65 508 B) and fails from C = 54 (66 960 B)."""
    N, C, P = dims(c)
    if 256 * C * 4 + C * C * 4 <= LDS and nhwc(strides(c["lay"], c["shape"]), N, C, P):
        return f"confusion_nhwc_kernel<{c['dt']}>"
    return "confusion_kernel"


def _cf(cid, shape, lay="cl", dt="f32", **kw):
    c = dict(op="confusion", id=f"confusion:{cid}", shape=shape, lay=lay, dt=dt, **kw)
    c["kernel"] = kw.get("kernel") or conf_rule(c)
    CASES.append(c)
    return c


for _dt in ("f32", "bf16"):
    _cf(f"nhwc-{_dt}", (2, 19, 9, 14), dt=_dt, kernel=f"confusion_nhwc_kernel<{_dt}>")
    _cf(f"nchw-{_dt}", (2, 19, 9, 14), lay="nchw", dt=_dt, kernel="confusion_kernel")
for _C in (51, 52, 53):
    _cf(f"C{_C}", (1, _C, 9, 31), kernel="confusion_nhwc_kernel<f32>", **({"gate": ("conf-lds", 0)} if _C == 53 else {}))
_cf("C54", (1, 54, 9, 31), kernel="confusion_kernel", gate=("conf-lds", 1))
_cf("C64", (1, 64, 9, 31), kernel="confusion_kernel")
_cf("cslice", (2, 19, 5, 7), lay="cs", kernel="confusion_kernel")
_cf("bslice-N1", (1, 19, 5, 7), lay="bs", kernel="confusion_nhwc_kernel<f32>")
_cf("accumulate", (2, 19, 9, 14), accumulate=True)
_cf("out-of-range", (2, 19, 9, 14), out_of_range=True)
_cf("second-trip-nhwc", (1, 3, 525, 1001), second_trip=(525 * 1001, MAX_BLOCKS))
_cf("second-trip-nchw", (3, 3, 175, 1001), lay="nchw", dt="bf16", second_trip=(3 * 175 * 1001, MAX_BLOCKS))


def confusion_of(x, y, C):
    """(C, C) [label][first argmax] over the labels inside [0, C); x (N, C, ...) float64."""
    pred = torch.argmax(x, 1).reshape(-1)
    y = y.reshape(-1)
    ok = (y >= 0) & (y < C)
    return torch.bincount(y[ok] * C + pred[ok], minlength=C * C).reshape(C, C).numpy().astype(np.int64)


def build_confusion(c):
    r = rng_of(c)
    N, C = c["shape"][:2]
    x = q(r.standard_normal(c["shape"]), c["dt"])
    y = labels_of(c, r, N, C, c["shape"][2:])
    conf = confusion_of(t64(x), torch.from_numpy(y), C)
    inp = {"x": x, "y": y}
    if c.get("accumulate"):
        inp["conf0"] = r.integers(0, 1000, size=(C, C)).astype(np.int64)
        conf = conf + inp["conf0"]
    return inp, {"conf": conf}


# ================================================================================ the five entry points on low-resolution logits
UP_LIMIT = {"ce2d_up": 48, "focal_up": 48, "metrics_up": 48, "kldiv_up": 24, "jsdiv_up": 24}
UP_CAP = {"ce2d_up": MAX_BLOCKS, "kldiv_up": MAX_BLOCKS, "jsdiv_up": MAX_BLOCKS, "focal_up": FOCAL_MAX_BLOCKS, "metrics_up": MET_MAX_BLOCKS}
UP_NAME = {"ce2d_up": "ce2d_up_kernel<{}>", "kldiv_up": "pair_up_kernel<kld,{}>", "jsdiv_up": "pair_up_kernel<jsd,{}>",
           "focal_up": "focal_up_kernel<{}>", "metrics_up": "logit_metrics_up_kernel<{}>"}


def up_rule(c):
    """loss_select_up: "if (C > loss_up_max_classes(op))" (48, or 24 for the two divergences), then (int)(255.f * c.sw) + 3 <=
    LOSS_UP_NW as "if (!(255.f * c.sw < (float)(LOSS_UP_NW - 2)))" (c.sw = (w - 1) / (W - 1) with align_corners, w / W without),
    then "LK_CE2D_UP_0 + 2 * op + (C == 19)": ..._kernel<19> or ..._kernel<0>.  None: the call is refused."""
    N, h, w, C, H, W = c["geom"]
    if C > UP_LIMIT[c["op"]]:
        return None
    sw = np.float32(w - 1) / np.float32(W - 1) if c["ac"] and W > 1 else (np.float32(0) if c["ac"] else np.float32(w) / np.float32(W))
    if int(np.float32(255.0) * sw) + 3 > UP_NW:
        return None
    return UP_NAME[c["op"]].format(19 if C == 19 else 0)


def up_chunks(c):
    """loss_select_up: "c.cpr = (W + 255) / 256; c.nchunks = (long long)N * H * c.cpr;" """
    N, h, w, C, H, W = c["geom"]
    return N * H * ((W + 255) // 256)


def _up(op, cid, geom, ac=True, **kw):
    c = dict(op=op, id=f"{op}:{cid}-{'ac' if ac else 'hp'}", geom=geom, ac=ac, **kw)
    c["kernel"] = up_rule(c)
    if c["kernel"] is None:
        c["refused"] = True
        c["kernel"] = "(refused)"
    CASES.append(c)
    return c


UP_INSIDE = "per-pixel values of order 1 over 17 000 pixels: a single chain stays far inside 1e-4"
for _op in UP_LIMIT:
    for _C in (18, 19, 20):
        _up(_op, f"C{_C}", (2, 5, 7, _C, 9, 14), ac=_C != 20, gate=("up-c19", _op, int(_C == 19)))
    _lim = UP_LIMIT[_op]
    _up(_op, f"C{_lim}", (1, 5, 7, _lim, 9, 14))
    _up(_op, f"C{_lim + 1}-refused", (1, 5, 7, _lim + 1, 9, 14))
    _up(_op, "ratio-refused", (1, 5, 200, 3, 5, 300))          # (int)(255 * 199 / 299) + 3 = 172 source columns
    _up(_op, "spread30", (2, 5, 7, 19, 9, 14), spread=30.0)
    _up(_op, "spread30-C5", (2, 5, 7, 5, 9, 14), ac=False, spread=30.0)
    for _ac in (True, False):
        # 2100 chunks of 8 pixels: above every cap (2048, 1365, 1024)
        _up(_op, "second-trip", (3, 350, 4, 3, 700, 8), ac=_ac, second_trip=(2100 * 256, UP_CAP[_op]),
            **({"chain": ("inside", UP_INSIDE)} if _op in ("ce2d_up", "kldiv_up", "jsdiv_up") else {}))
        _up(_op, "W257", (1, 3, 129, 19 if _ac else 5, 5, 257), ac=_ac)     # two chunks a row, the second one pixel wide
        _up(_op, "W511", (1, 3, 200, 5 if _ac else 19, 5, 511), ac=_ac)     # the second 255 pixels wide


_up("ce2d_up", "all-ignored", (2, 5, 7, 19, 9, 14), all_ignored=True)
_up("metrics_up", "all-ignored", (2, 5, 7, 5, 9, 14), all_ignored=True)


def interp64(x_lo, size, ac):
    """(N, h, w, C) -> (N, C, H, W) float64, F.interpolate's bilinear."""
    return F.interpolate(t64(x_lo).permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=ac)


def near_tie(x, tol):
    """(N, H, W) mask of the pixels of x (N, C, H, W) whose two best classes lie within tol of each other without being equal."""
    v = torch.topk(x, 2, dim=1).values
    g = v[:, 0] - v[:, 1]
    return (g > 0) & (g < tol)


def build_up(c):
    op = c["op"]
    N, h, w, C, H, W = c["geom"]
    r = rng_of(c)
    draw = (lambda: r.uniform(-c["spread"], c["spread"], (N, h, w, C))) if "spread" in c else (lambda: r.standard_normal((N, h, w, C)) * 2)
    s, t = draw().astype(np.float32), draw().astype(np.float32)
    c2 = dict(c, ignore_index=255 if op != "focal_up" else -100)
    y = labels_of(c2, r, N, C, (H, W))
    inp = {"s": s, "t": t, "y": y}
    if c.get("refused"):
        return inp, {}
    S, T = interp64(s, (H, W), c["ac"]), interp64(t, (H, W), c["ac"])
    if op == "metrics_up":
        # The confusion matrices are compared exactly, and the kernel forms a pixel's source coordinate in fp32 (up_chunk / up_col:
        # "fmaxf(wo * g.sw + g.ow, 0.f)" with g.sw rounded too): three roundings at a magnitude of up to max(h, w), so each of the
        # two blends moves a value by up to 3u * max(h, w) * (the logits' range), and the gap between two classes by twice that
        # -- plus the blends' own few ulp.  A pixel whose two best classes are closer than that in either tensor could land on
        # either class: it gets the label 255, outside [0, C), and is counted by nothing (a tie proper stays: the first
        # maximum wins on both sides).
        span = float(max(np.ptp(s), np.ptp(t)))
        tol = 12 * U * max(h, w) * span + 16 * U * span
        y[(near_tie(S, tol) | near_tie(T, tol)).numpy()] = 255
        inp["near_ties"] = int((y == 255).sum())
    yt = torch.from_numpy(y)
    if op == "ce2d_up":
        nll, tot, loss, _ = ce_formula(S, yt, None, True, 255)
        return inp, {"loss": float(loss), "terms": nll.numpy().ravel(), "scale": 1.0 / max(float(tot), 1e-300)}
    if op in ("kldiv_up", "jsdiv_up"):
        vals, scale, _ = pair_formula("kld" if op == "kldiv_up" else "jsd", S, T, 2.0)
        return inp, {"loss": float(vals.sum() * scale), "terms": vals.numpy().ravel(), "scale": scale}
    if op == "focal_up":
        alpha = (np.abs(r.standard_normal(C)) + 0.2).astype(np.float32)
        inp["alpha"] = alpha
        ref = {}
        for red in ("mean", "sum"):
            ref[red] = float(CR.focal(S, yt, 2.0, torch.from_numpy(alpha), -100, red)[0])
        ref["stats"] = focal_maps(S, yt, 2.0, alpha, -100)[2]
        return inp, ref
    ce_s, ce_t = float(ce_formula(S, yt, None, True, 255)[2]), float(ce_formula(T, yt, None, True, 255)[2])
    return inp, {"out": np.array([ce_s, ce_t, float(((S - T) ** 2).mean())]), "conf_s": confusion_of(S, yt, C), "conf_t": confusion_of(T, yt, C)}


# ============================================================================================================ focal and its gradient
def focal_maps(x, y, gamma_, alpha, ignore_index):
    """(a_map, ce_map, stats) of losses/FocalLoss.py:15-28 as kd_focal lays them out: a = (1 - p_y')^gamma with y' = y at valid
    pixels and 0 elsewhere, ce = alpha_y * -log p_y at valid pixels and 0 elsewhere, stats = (sum a, sum ce, sum alpha_y)."""
    N, C = x.shape[:2]
    xs, tg = x.reshape(N, C, -1), y.reshape(N, -1)
    valid = (tg != ignore_index) & (tg >= 0) & (tg < C)
    yv = torch.where(valid, tg, torch.zeros_like(tg))
    lp = F.log_softmax(xs, 1)
    py = lp.exp().gather(1, yv[:, None])[:, 0]
    a = (1 - py) ** gamma_
    w = torch.ones(C, dtype=torch.float64) if alpha is None else t64(alpha)
    wy = torch.where(valid, w[yv], torch.zeros_like(py))
    ce = -wy * lp.gather(1, yv[:, None])[:, 0]
    return a.numpy(), ce.numpy(), np.array([float(a.sum()), float(ce.sum()), float(wy.sum())])


def _focal(op, cid, shape, lay="cl", dt="f32", red="mean", gamma_=2.0, **kw):
    return case(op, cid, "focal_kernel" if op == "focal" else "focal_grad_kernel", shape=shape, lay=lay, dt=dt, red=red, gamma=gamma_, **kw)


for _op in ("focal", "focal_grad"):
    for _red in ("mean", "sum", "none"):
        _focal(_op, f"{_red}-cl", (2, 19, 9, 14), red=_red, alpha=True)
        _focal(_op, f"{_red}-nchw", (2, 19, 9, 14), lay="nchw", red=_red, maps=_red == "none")   # (mean / sum without the maps: training)
    _focal(_op, "bf16", (2, 19, 9, 14), dt="bf16", alpha=True)
    _focal(_op, "gamma0", (2, 19, 9, 14), gamma_=0.0)
    _focal(_op, "gamma-half", (2, 19, 9, 14), gamma_=0.5, alpha=True)
    _focal(_op, "cslice", (2, 19, 5, 7), lay="cs")
    _focal(_op, "spread30", (2, 19, 9, 14), spread=30.0)
    _focal(_op, "out-of-range", (2, 19, 9, 14), lay="nchw", out_of_range=True)
# 525 525 pixels: above focal's 1365-block cap and the gradient's 2048
_focal("focal", "second-trip", (1, 3, 525, 1001), maps=False, second_trip=(525 * 1001, FOCAL_MAX_BLOCKS), chain=("inside", CE_INSIDE))
_focal("focal", "second-trip-maps", (1, 3, 525, 1001), second_trip=(525 * 1001, FOCAL_MAX_BLOCKS), chain=("inside", CE_INSIDE))
_focal("focal_grad", "second-trip", (1, 3, 525, 1001), second_trip=(525 * 1001, MAX_BLOCKS))


def build_focal(c):
    r = rng_of(c)
    shape = c["shape"]
    N, C = shape[:2]
    x = q(r.uniform(-c["spread"], c["spread"], shape) if "spread" in c else r.standard_normal(shape) * 2, c["dt"])
    y = labels_of(dict(c, ignore_index=-100), r, N, C, shape[2:])
    alpha = (np.abs(r.standard_normal(C)) + 0.2).astype(np.float32) if c.get("alpha") else None
    P = int(np.prod(shape[2:]))
    up = (r.standard_normal((N, N) + tuple(shape[2:])) if c["red"] == "none" else np.array(0.75)).astype(np.float32)
    X, Y = t64(x), torch.from_numpy(y)
    loss, grad = CR.focal(X, Y, c["gamma"], None if alpha is None else torch.from_numpy(alpha), -100, c["red"], torch.from_numpy(up))
    a, ce, stats = focal_maps(X, Y, c["gamma"], alpha, -100)
    ref = {"loss": loss.numpy() if c["red"] == "none" else float(loss), "grad": grad.numpy(), "a_map": a.reshape(N, P), "ce_map": ce.reshape(N, P),
           "stats": stats, "terms": ce.ravel(), "scale": 1.0}
    return {"x": x, "y": y, "alpha": alpha, "up": up}, ref


# ========================================================================================================== kd_topk_hint_mse
def topk_rule(c):
    """loss_select_topk: no gradient -> "topk_nograd"; "const bool cfast = s->sC == 1 && s->sP == C;"
    "if (loss_dense_same(s, t, grad, N, C, P) && (cfast ? C % 8 == 0 : P % 8 == 0) && (mk & 15u) == 0)" -> topk_grad_vec_kernel<T, CF>,
    else topk_grad_kernel.  (mk: the caller's (N, C) fp32 mask or the workspace's own, both 16-B aligned here.)"""
    N, C, P = dims(c)
    if not c.get("gdt", c["sdt"]):
        return "topk_nograd"
    st = strides(lays(c)[0], c["shape"])
    cfast = st[1] == 1 and st[2] == C
    if dense_same(c) and (C % 8 == 0 if cfast else P % 8 == 0):
        return f"topk_grad_vec_kernel<{c['sdt']},{'cfast' if cfast else 'pfast'}>"
    return "topk_grad_kernel"


def _tk(cid, shape, lay="cl", dt="f32", k=None, **kw):
    c = dict(op="topk", id=f"topk:{cid}", shape=shape, lay=lay, sdt=dt, tdt=dt, k=shape[1] // 2 if k is None else k, **kw)
    c.setdefault("gdt", dt)
    c["kernel"] = kw.get("kernel") or topk_rule(c)
    CASES.append(c)
    return c


for _dt in ("f32", "bf16"):
    _tk(f"cfast-C24-{_dt}", (2, 24, 5, 7), dt=_dt, kernel=f"topk_grad_vec_kernel<{_dt},cfast>", gate=("topk-c8", _dt, 0))
    _tk(f"cfast-C20-{_dt}", (2, 20, 4, 6), dt=_dt, kernel="topk_grad_kernel", gate=("topk-c8", _dt, 1))     # numel % 8 = 0, C % 8 = 4
    _tk(f"pfast-P40-{_dt}", (2, 21, 5, 8), lay="nchw", dt=_dt, kernel=f"topk_grad_vec_kernel<{_dt},pfast>", gate=("topk-p8", _dt, 0))
    _tk(f"pfast-P36-{_dt}", (2, 22, 6, 6), lay="nchw", dt=_dt, kernel="topk_grad_kernel", gate=("topk-p8", _dt, 1))   # numel % 8 = 0, P % 8 = 4
_tk("cslice-g", (2, 24, 5, 7), lay=("cl", "cl", "cs"), kernel="topk_grad_kernel")
_tk("nograd", (2, 24, 5, 7), gdt=None, kernel="topk_nograd")
_tk("k1", (2, 24, 5, 7), k=1)
_tk("kC", (2, 24, 5, 7), k=24)
_tk("C70-two-channel-groups", (3, 70, 9, 11), lay="nchw", k=17)
_tk("tie", (2, 24, 5, 7), k=12, tie=True)           # two target channels are equal and straddle rank k
_tk("tie-nchw", (2, 24, 5, 8), lay="nchw", k=12, tie=True)
_tk("K0-refused", (2, 24, 5, 7), k=0, refused=True, kernel="(refused)")
_tk("K25-refused", (2, 24, 5, 7), k=25, refused=True, kernel="(refused)")
# 4 204 032 elements: 525 504 octets, above the 2048 x 256 grid of either gradient kernel
_tk("second-trip-vec", (1, 8, 513, 1024), k=4, second_trip=(513 * 1024, MAX_BLOCKS), chain=("inside", "the kernel reduces per channel in fp64; the loss adds 4 channel sums"))
_tk("second-trip-strided", (1, 4, 131251, 1), lay="nchw", k=2, second_trip=(525004, MAX_BLOCKS), chain=("inside", "as the vector row"))


def build_topk(c):
    r = rng_of(c)
    shape = c["shape"]
    N, C = shape[:2]
    s = q(r.standard_normal(shape), c["sdt"])
    # channel norms apart by construction: channel c of sample n is rescaled to the norm 1.03^k, k a permutation of 0 .. C - 1,
    # so neighbouring squared norms differ by 6 %; rounding to bf16 moves a squared norm by 2^-8 = 0.4 % at most
    t = r.standard_normal(shape).reshape(N, C, -1)
    want = 1.03 ** np.stack([r.permutation(C) for _ in range(N)]).astype(np.float64)
    t = q((t * (want / np.sqrt((t * t).sum(-1)))[:, :, None]).reshape(shape), c["tdt"])
    if c.get("tie"):
        # the channel of rank k + 1 becomes a copy of the channel of rank k: the two tie exactly for the last kept place (every
        # other rank is as it was), and the lower channel of the two must win it
        order = np.argsort(-(t.astype(np.float64) ** 2).reshape(N, C, -1).sum(-1), axis=1, kind="stable")
        for n in range(N):
            t[n, order[n, c["k"]]] = t[n, order[n, c["k"] - 1]]
        inp_tie = [tuple(sorted((int(order[n, c["k"] - 1]), int(order[n, c["k"]])))) for n in range(N)]
    inp = {"s": s, "t": t, "k": c["k"]}
    if c.get("tie"):
        inp["tie"] = inp_tie
    if c.get("refused"):
        return inp, {}
    S, T = t64(s), t64(t)
    if len(shape) == 2:
        S, T = S[:, :, None, None], T[:, :, None, None]
    loss, grad = CR.topk_hint(S, T, (c["k"] + 0.5) / C)
    mask, k = CR.topk_mask(T, (c["k"] + 0.5) / C)
    assert k == c["k"]
    d2 = ((S - T) ** 2).reshape(N, C, -1).sum(-1) * mask
    ref = {"loss": float(loss), "mask": mask.numpy(), "terms": d2.numpy().ravel(), "scale": 1.0 / (S[0, 0].numel() * N * k)}
    if c.get("gdt"):
        ref["grad"] = grad.reshape(shape).numpy()
    return inp, ref


# ============================================================================================ kd_kldiv_multi / kd_softmax_mean
def row_vec_ok(lay, dt, shape):
    """loss_select.h loss_row_vec_ok(): "(C & 3) == 0 && ((uintptr_t)v->ptr & (v->dtype == KD_BF16 ? 7u : 15u)) == 0 && (P == 1 ||
    (v->sP & 3) == 0) && (N == 1 || (v->sN & 3) == 0)" """
    N, C, P = (shape[0], shape[1], 1) if len(shape) == 2 else (shape[0], shape[1], shape[2] * shape[3])
    sN, sC, sP = strides(lay, shape)
    base_ok = lay != "off1"        # a slice starts 8 elements in: 32 B of fp32, 16 B of bf16
    return C % 4 == 0 and base_ok and (P == 1 or sP % 4 == 0) and (N == 1 or sN % 4 == 0)


def multi_rule(c):
    """loss_select_multi: "bool unit = (!s || s->sC == 1) && (!g || g->sC == 1);" (and every target's), "bool dense = !smean &&
    (!s || loss_nhwc(s, N, C, P)) && (!g || loss_nhwc(g, N, C, P));" (and every target's), vec = loss_row_vec_ok of all of them;
    "const bool narrow = C < 22 && rows >= 16384;"
    "if (narrow && dense)" -> kldm_nhwc_kernel, "else if (unit && C <= 1024 && !narrow)" -> the wave kernel
    "LK_MT_WAVE_1_VEC + 4 * smean + 2 * (C > 256) + !vec", else kldm_kernel / kldm_kernel<smean>.
    kd_softmax_mean asks the same function without a student and with smean (no NHWC kernel for it)."""
    N, C, P = dims(c)
    rows = N * P
    smean = c["op"] == "softmax_mean"
    # every operand of a row has the row's layout (the wrappers allocate the gradient / the fp32 output like the first operand,
    # dense in the same order: the same answers to the three questions below)
    ops_ = [(c["lay"], c["dt"])] * (c["nt"] + 1)
    unit = all(strides(l, c["shape"])[1] == 1 for l, _ in ops_)
    dense = all(nhwc(strides(l, c["shape"]), N, C, P) for l, _ in ops_)
    vec = all(row_vec_ok(l, d, c["shape"]) for l, d in ops_)
    narrow = C < 22 and rows >= 16384
    tail = ",smean>" if smean else ">"
    if not smean and narrow and dense:
        return "kldm_nhwc_kernel"
    if unit and C <= 1024 and not narrow:
        return f"mt_wave_kernel<{1 if C <= 256 else 4},{'vec' if vec else 'novec'}{tail}"
    return "kldm_kernel<smean>" if smean else "kldm_kernel"


def _mt(op, cid, shape, lay="2d", dt="f32", nt=2, **kw):
    c = dict(op=op, id=f"{op}:{cid}", shape=shape, lay=lay, dt=dt, nt=nt, **kw)
    c["kernel"] = multi_rule(c)
    if "expect" in kw:
        assert c["kernel"].startswith(kw["expect"]), (c["id"], c["kernel"])
    CASES.append(c)
    return c


for _op in ("kldiv_multi", "softmax_mean"):
    _mt(_op, "C100-vec", (9, 100), expect="mt_wave_kernel<1,vec")                     # rows % 4 = 1
    _mt(_op, "C100-vec-bf16", (9, 100), dt="bf16", expect="mt_wave_kernel<1,vec")
    _mt(_op, "C10-novec", (37, 10), expect="mt_wave_kernel<1,novec")
    _mt(_op, "C100-slice-vec", (9, 100), lay="2ds", expect="mt_wave_kernel<1,vec")     # rows of a wider buffer, still 4-aligned
    _mt(_op, "C256", (5, 256), expect="mt_wave_kernel<1,vec", gate=("mt-c256", _op, 0))
    _mt(_op, "C260", (5, 260), expect="mt_wave_kernel<4,vec", gate=("mt-c256", _op, 1))
    _mt(_op, "C258-novec", (5, 258), expect="mt_wave_kernel<4,novec")
    _mt(_op, "C300-bf16", (5, 300), dt="bf16", expect="mt_wave_kernel<4,vec")
    _mt(_op, "C1024", (5, 1024), expect="mt_wave_kernel<4,vec", gate=("mt-c1024", _op, 0))
    _mt(_op, "C1028", (5, 1028), expect="kldm_kernel", gate=("mt-c1024", _op, 1))
    _mt(_op, "nchw-any", (2, 19, 9, 14), lay="nchw", expect="kldm_kernel")              # class stride P
    _mt(_op, "cl-wave", (2, 19, 9, 14), lay="cl", nt=3, expect="mt_wave_kernel<1,novec")
    _mt(_op, "cl-wave-C24", (2, 24, 9, 14), lay="cl", expect="mt_wave_kernel<1,vec")
    _mt(_op, "cslice-wave", (2, 24, 5, 7), lay="cs", expect="mt_wave_kernel<1,vec")
    # narrow: C < 22 and rows >= 16384 (128 x 128 pixels); both neighbours of each threshold
    _mt(_op, "C21-rows16384", (1, 21, 128, 128), lay="cl", expect="kldm_nhwc_kernel" if _op == "kldiv_multi" else "kldm_kernel<smean>", gate=("mt-narrow-c", _op, 0))
    _mt(_op, "C22-rows16384", (1, 22, 128, 128), lay="cl", expect="mt_wave_kernel<1,novec", gate=("mt-narrow-c", _op, 1),
        second_trip=(16384 * 64, MT_MAX_BLOCKS), chain=("inside", "16 384 per-pixel values of order 0.1"))       # 4096 blocks of 4 rows > 1365
    _mt(_op, "C19-rows16383", (1, 19, 127, 129), lay="cl", expect="mt_wave_kernel<1,novec", gate=("mt-narrow-rows", _op, 0))
    _mt(_op, "C19-rows16384", (1, 19, 128, 128), lay="cl", expect="kldm_nhwc_kernel" if _op == "kldiv_multi" else "kldm_kernel<smean>", gate=("mt-narrow-rows", _op, 1))
    _mt(_op, "C19-rows16384-nchw", (1, 19, 128, 128), lay="nchw", expect="kldm_kernel")   # narrow but not dense
    # batch slices (sN != C * P): dense only through nhwc_dense's "|| N == 1"
    _mt(_op, "C19-rows16384-bslice-N1", (1, 19, 128, 128), lay="bs", expect="kldm_nhwc_kernel" if _op == "kldiv_multi" else "kldm_kernel<smean>")
    _mt(_op, "C19-rows16384-bslice-N2", (2, 19, 64, 128), lay="bs", expect="kldm_kernel")
    _mt(_op, "wave-second-trip-tail", (5465, 24), expect="mt_wave_kernel<1,vec", second_trip=(5465 * 64, MT_MAX_BLOCKS),
        chain=("inside", "5465 per-row values of order 0.1"))                                # 1367 blocks of 4 rows, rows % 4 = 1
_mt("kldiv_multi", "nograd", (9, 100), grad=False)
_mt("kldiv_multi", "nolabels", (9, 100), labels=False)
_mt("kldiv_multi", "T1", (9, 100), T=1.0)
_mt("kldiv_multi", "nhwc-bf16", (1, 19, 128, 128), lay="cl", dt="bf16", expect="kldm_nhwc_kernel")
_mt("kldiv_multi", "nhwc-second-trip", (1, 3, 525, 1001), lay="cl", nt=1, expect="kldm_nhwc_kernel", second_trip=(525 * 1001, MT_MAX_BLOCKS),
    chain=("inside", CE_INSIDE))
_mt("kldiv_multi", "any-second-trip", (1, 3, 525, 1001), lay="nchw", nt=1, expect="kldm_kernel", second_trip=(525 * 1001, MT_MAX_BLOCKS),
    chain=("inside", CE_INSIDE))
_mt("softmax_mean", "any-second-trip", (1, 3, 525, 1001), lay="cl", nt=1, expect="kldm_kernel<smean>", second_trip=(525 * 1001, MT_MAX_BLOCKS))
for _op in ("kldiv_multi", "softmax_mean"):
    case(_op, "0-targets-refused", "(refused)", shape=(9, 100), lay="2d", dt="f32", nt=0, refused=True)
    case(_op, "17-targets-refused", "(refused)", shape=(9, 100), lay="2d", dt="f32", nt=17, refused=True)


def build_multi(c):
    r = rng_of(c)
    shape = c["shape"]
    N, C = shape[:2]
    nt = min(max(c["nt"], 1), 3) if c.get("refused") else c["nt"]
    s = q(r.standard_normal(shape) * 2, c["dt"])
    ts = [q(r.standard_normal(shape) * 2, c["dt"]) for _ in range(nt)]
    w = [0.5 + k for k in range(nt)]
    y = labels_of(c, r, N, C, shape[2:]) if c.get("labels", True) else None
    T = c.get("T", 3.0)
    inp = {"s": s, "ts": ts, "w": w, "y": y, "T": T, "kd_scale": 0.7, "sup_scale": 1.3}
    if c.get("refused"):
        return inp, {}
    if c["op"] == "softmax_mean":
        return inp, {"out": ER.softmax_mean([t64(t) for t in ts], w, T).numpy()}
    o = ER.kldiv_multi(t64(s), [t64(t) for t in ts], w, T, None if y is None else torch.from_numpy(y), 255, 0.7, 1.3)
    lps = F.log_softmax(t64(s) / T, 1)
    terms = sum((wk / sum(w)) * (lambda pt: (torch.xlogy(pt, pt) - pt * lps).sum(1))(torch.softmax(t64(t) / T, 1)) for wk, t in zip(w, ts))
    return inp, {"kd": float(o["kd"]), "sup": float(o["sup"]), "total": float(o["total"]), "grad": o["grad"].numpy(),
                 "terms": terms.numpy().ravel(), "scale": T * T / terms.numel()}


# ================================================================================================= kd_radam_step / kd_radam_step_multi
def radam_constants(step, beta1, beta2):
    """utils/optim/radam.py _rect(): (rectified, step_size)."""
    b2t = beta2 ** step
    nmax = 2.0 / (1.0 - beta2) - 1.0
    nsma = nmax - 2.0 * step * b2t / (1.0 - b2t)
    if nsma >= 5.0:
        return True, math.sqrt((1 - b2t) * (nsma - 4) / (nmax - 4) * (nsma - 2) / nsma * nmax / (nmax - 2)) / (1 - beta1 ** step)
    return False, 1.0 / (1 - beta1 ** step)


# beta2 = 0.999: N_sma = 0.999, 4.98 | 5.97, 6.96 at steps 1, 5 | 6, 7
for _step in (1, 5, 6, 7):
    for _wd in (0.0, 1e-2):
        for _n in (1, 2049):       # one element; one past a block of the multi-tensor kernel (and nine blocks of the single one)
            case("radam", f"step{_step}-wd{_wd:g}-n{_n}", "radam_kernel", step=_step, wd=_wd, n=_n, rect=_step >= 6)
case("radam", "second-trip", "radam_kernel", step=7, wd=1e-2, n=525001, rect=True, second_trip=(525001, MAX_BLOCKS))
case("radam_multi", "eight-tensors", "radam_multi_kernel", items=[(s, w, n) for s in (1, 5, 6, 7) for w, n in ((0.0, 2049), (1e-2, 1))])
case("radam_multi", "fifty-tensors", "radam_multi_kernel", items=[(1 + i % 7, 1e-2 * (i % 2), 1 + 41 * i) for i in range(50)])   # two launches of 48 + 2


def radam_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd):
    """utils/optim/radam.py:74-89 in float64 -> (p, m, v)."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    v = v * beta2 + (1 - beta2) * g * g
    m = m * beta1 + (1 - beta1) * g
    rect, ss = radam_constants(step, beta1, beta2)
    if wd != 0:
        p = p + -wd * lr * p
    p = p + (-ss * lr * m / (np.sqrt(v) + eps) if rect else -ss * lr * m)
    return p, m, v


RADAM_HP = dict(lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8)


def radam_tensor(r, n, step, wd):
    p, g = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    m = (r.standard_normal(n) * 0.1).astype(np.float32) if step > 1 else np.zeros(n, np.float32)
    v = (np.abs(r.standard_normal(n)) * 0.01).astype(np.float32) if step > 1 else np.zeros(n, np.float32)
    return dict(p=p, g=g, m=m, v=v, step=step, wd=wd), radam_ref(p, g, m, v, step, wd=wd, **RADAM_HP)


def build_radam(c):
    r = rng_of(c)
    items = [(c["step"], c["wd"], c["n"])] if c["op"] == "radam" else c["items"]
    built = [radam_tensor(r, n, step, wd) for step, wd, n in items]
    return {"tensors": [b[0] for b in built]}, {"tensors": [b[1] for b in built]}


# ================================================================================================ kd_scale_by_device_scalar
for _dt in ("f32", "bf16"):
    for _n in (1, 7, 8, 9, 10, 11, 12, 13, 14, 15, 2048 * 8 + 3):
        case("scale", f"n{_n}-{_dt}", f"scale_by_device_scalar_kernel<{_dt}>", n=_n, dt=_dt, scale=0.375)
    case("scale", f"one-{_dt}", f"scale_by_device_scalar_kernel<{_dt}>", n=77, dt=_dt, scale=1.0)       # leaves at once: a move
case("scale", "second-trip-f32", "scale_by_device_scalar_kernel<f32>", n=525001 * 8 + 5, dt="f32", scale=0.375, second_trip=(525001, MAX_BLOCKS))


def build_scale(c):
    x = q(rng_of(c).standard_normal(c["n"]), c["dt"])
    return {"x": x, "scale": c["scale"]}, {"y": x.astype(np.float64) * c["scale"]}


# ====================================================================================================================== build
BUILDERS = {"pair": build_pair, "hint_mse": build_mse, "whmse": build_whmse, "ce2d": build_ce, "ce2d_grad": build_ce, "confusion": build_confusion,
            "ce2d_up": build_up, "kldiv_up": build_up, "jsdiv_up": build_up, "focal_up": build_up, "metrics_up": build_up,
            "focal": build_focal, "focal_grad": build_focal, "topk": build_topk, "kldiv_multi": build_multi, "softmax_mean": build_multi,
            "radam": build_radam, "radam_multi": build_radam, "scale": build_scale}
RULES = {"pair": pair_rule, "hint_mse": mse_rule, "ce2d": ce_rule, "confusion": conf_rule, "topk": topk_rule, "kldiv_multi": multi_rule,
         "softmax_mean": multi_rule, "ce2d_up": up_rule, "kldiv_up": up_rule, "jsdiv_up": up_rule, "focal_up": up_rule, "metrics_up": up_rule}


def build(c):
    """-> (inputs, reference): dicts of numpy arrays (inputs rounded to the storage dtype, references float64)."""
    return BUILDERS[c["op"]](c)


def rule(c):
    """The name the family's selector, restated above, picks for the row ("(refused)" when nothing is launched); entry points
    with one kernel have no gate to restate."""
    op = c["op"]
    if op == "topk" and not 1 <= c["k"] <= c["shape"][1]:       # "KD_REQUIRE(K >= 1 && K <= C, ...)"
        return "(refused)"
    if op in ("kldiv_multi", "softmax_mean") and not 1 <= c["nt"] <= KD_MULTI_MAX:    # mt_pack: "ts->n < 1 || ts->n > KD_MULTI_MAX"
        return "(refused)"
    r = RULES.get(op)
    return (r(c) or "(refused)") if r else c["kernel"]


def expected_shapes(c):
    """{reference name: shape} of the array-valued references of a row."""
    op = c["op"]
    if c.get("refused"):
        return {}
    if op in ("pair", "hint_mse", "whmse", "topk"):
        out = {"grad": c["shape"]} if c.get("gdt") else {}
        if op == "topk":
            out["mask"] = c["shape"][:2]
        return out
    if op in ("ce2d", "ce2d_grad"):
        return {"grad": c["shape"]}
    if op == "confusion":
        return {"conf": (c["shape"][1],) * 2}
    if op == "metrics_up":
        return {"out": (3,), "conf_s": (c["geom"][3],) * 2, "conf_t": (c["geom"][3],) * 2}
    if op in ("focal", "focal_grad"):
        N, P = c["shape"][0], int(np.prod(c["shape"][2:]))
        return {"grad": c["shape"], "a_map": (N, P), "ce_map": (N, P), "stats": (3,)}
    if op == "kldiv_multi":
        return {"grad": c["shape"]}
    if op == "softmax_mean":
        return {"out": c["shape"]}
    if op == "scale":
        return {"y": (c["n"],)}
    return {}


def shrunk(c):
    """A second-trip row with a short plane (the same reference path in a fraction of the time), for the host test."""
    if "second_trip" not in c:
        return c
    if "geom" in c:
        N, h, w, C, H, W = c["geom"]
        return dict(c, geom=(N, 6, w, C, 12, W))
    if "shape" in c and len(c["shape"]) == 4:
        N, C, H, W = c["shape"]
        return dict(c, shape=(N, C, min(H, 8), W))
    if "shape" in c:
        return dict(c, shape=(min(c["shape"][0], 41), c["shape"][1]))
    if "n" in c:
        return dict(c, n=min(c["n"], 4099))
    return c


# ============================================================================= what a single fp32 chain would do to each reduction
REDUCTIONS = ("pair", "hint_mse", "whmse", "ce2d", "ce2d_up", "kldiv_up", "jsdiv_up", "focal", "topk", "kldiv_multi")


def chain32(terms):
    """Sequential fp32 accumulation of `terms` (rounded to fp32 first), in order."""
    return float(np.cumsum(np.asarray(terms, dtype=np.float32).ravel(), dtype=np.float32)[-1])


def loss_bound(c, ref):
    """The bound the scalar of a row is held to: the project's rtol = 1e-4, or the recursive-summation bound where the row has one."""
    return ref.get("bound", 1e-4 * abs(ref["loss"] if "loss" in ref else ref["kd"]))


def single_chain(c, ref):
    """(error of ONE fp32 chain over the row's addends, the bound the kernel's two-stage reduction is held to)."""
    val = ref["loss"] if "loss" in ref else ref["kd"]
    if c["op"] == "focal":
        val = ref["stats"][1]
        return abs(chain32(ref["terms"]) - val), 1e-4 * abs(val)
    return abs(chain32(ref["terms"]) * ref["scale"] - val), loss_bound(c, ref)
